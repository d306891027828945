// Prediction: a real model image -> visibilities, the other half of a major cycle (include/gridhip.h, "predict").
// For every imaging function A (visibilities -> N x N grid) the prediction is its exact adjoint applied to the
// centred forward transform of the model, pred = A^H fft_c(model):
//   simple   the nearest cell of `grid` (src/Gridding.hs:95-112) read back: simple_degrid_kernel
//   conv     degrid2 with conj(kv)                (conv_imaging grids with kv)
//   w_cache  degrid2 with the w-kernels themselves (w_cache_imaging grids with their conjugates, :441)
//   aw       awdegrid with conj(wkerns), conj(akerns)
// and vis_out = pred, or vis_sub - pred (the residual).
//
// The transform: fft_c = shift2D . fft2D . ishift2D.  predict_head_kernel reads the real model once and writes the
// FFT's complex input with the ishift2D roll folded into its loads; for even N it also multiplies by (-1)^(y+x),
// which by the shift theorem is the shift2D after the transform, so the gathers read the FFT's output directly.
// For odd N that phase is not +-1, and the shift stays a roll after the transform.
#include "common.h"
#include "imaging.h"

namespace gridhip {

// out[y][x] = model[(y+s) mod N][(x+s) mod N] (imaginary part 0), negated where y + x is odd when `alt`
__global__ void __launch_bounds__(256) predict_head_kernel(int64_t N, const double *__restrict__ model,
                                                           double2 *__restrict__ out, int64_t s, int alt)
{
    const int64_t cells = N * N;
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < cells; c += (int64_t)gridDim.x * blockDim.x) {
        const int64_t y = c / N, x = c - y * N;
        int64_t sy = y + s, sx = x + s;
        sy -= sy >= N ? N : 0;
        sx -= sx >= N ? N : 0;
        const double m = model[sy * N + sx];
        out[c] = make_double2(alt && ((y + x) & 1) ? -m : m, 0.0);
    }
}

// The gather of simple_grid_kernel (simple.hip) with p = u / lam folded in (scale_kernel's division): the cell
// `grid` adds a visibility to is the cell it predicts from; where `grid` drops it (NaN, out of the grid) it predicts 0.
// n is the grid height for both axes (:101-103), as there.
__global__ void __launch_bounds__(256) simple_degrid_kernel(int64_t H, int64_t Wd, const double2 *__restrict__ grid,
                                                            int64_t n, const double *__restrict__ u,
                                                            const double *__restrict__ v, int64_t stride, double lam,
                                                            double2 *__restrict__ out)
{
#pragma clang fp contract(off)
    const int64_t halfn = H / 2;
    const double nf = (double)H;
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x) {
        const double pu = u[k * stride] / lam, pv = v[k * stride] / lam;
        double2 r = make_double2(0.0, 0.0);
        if (pu == pu && pv == pv) {
            const double fx = floor(0.5 + nf * pu), fy = floor(0.5 + nf * pv);
            if (fabs(fx) < 4.0e18 && fabs(fy) < 4.0e18) {
                const int64_t x = halfn + (int64_t)fx, y = halfn + (int64_t)fy;
                if (x >= 0 && y >= 0 && x < Wd && y < H) r = grid[y * Wd + x];
            }
        }
        out[k] = r;
    }
}

__global__ void __launch_bounds__(256) conj_copy_kernel(int64_t n, const double2 *__restrict__ in, double2 *__restrict__ out)
{
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x) {
        const double2 a = in[k];
        out[k] = make_double2(a.x, -a.y);
    }
}

// out = sub - pred, or pred when sub is null; sub may be out (an in-place residual): no __restrict__ on either
__global__ void __launch_bounds__(256) residual_kernel(int64_t n, const double2 *__restrict__ pred, const double2 *sub,
                                                       double2 *out)
{
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x) {
        const double2 p = pred[k];
        if (sub) {
            const double2 s = sub[k];
            out[k] = make_double2(s.x - p.x, s.y - p.y);
        } else
            out[k] = p;
    }
}

// F = fft_c(model) into f; t: scratch for odd N (unused for even N); plan: the caller's own transform, or the context's
int model_transform_to(gridhip_ctx *ctx, int64_t N, const double *model, double2 *f, double2 *t, void *plan)
{
    const size_t cells = (size_t)N * N;
    const bool even = N % 2 == 0;
    if (plan)
        GH_CHECK(fft_plan_bind(ctx, plan));
    else
        GH_CHECK(fft_plan_for(ctx, N, &plan));
    double2 *in = even ? f : t;
    hipLaunchKernelGGL(predict_head_kernel, grid_for(ctx, cells), dim3(256), 0, ctx->stream, N, model, in, N / 2,
                       even ? 1 : 0);
    GH_CHECK_HIP(ctx, hipGetLastError());
    GH_CHECK(fft_exec(ctx, plan, in, false));
    if (!even) GH_CHECK(launch_roll(ctx, N, in, f, (N + 1) / 2, 1.0));
    return GRIDHIP_OK;
}

int launch_simple_degrid(gridhip_ctx *ctx, int64_t H, int64_t Wd, const double2 *grid, int64_t n, const double *u,
                         const double *v, int64_t stride, double lam, double2 *out)
{
    hipLaunchKernelGGL(simple_degrid_kernel, grid_for(ctx, n), dim3(256), 0, ctx->stream, H, Wd, grid, n, u, v, stride, lam,
                       out);
    GH_CHECK_HIP(ctx, hipGetLastError());
    return GRIDHIP_OK;
}

int launch_conj_copy(gridhip_ctx *ctx, int64_t n, const double2 *in, double2 *out)
{
    hipLaunchKernelGGL(conj_copy_kernel, grid_for(ctx, n), dim3(256), 0, ctx->stream, n, in, out);
    GH_CHECK_HIP(ctx, hipGetLastError());
    return GRIDHIP_OK;
}

int launch_residual(gridhip_ctx *ctx, int64_t n, const double2 *pred, const double2 *sub, double2 *out)
{
    hipLaunchKernelGGL(residual_kernel, grid_for(ctx, n), dim3(256), 0, ctx->stream, n, pred, sub, out);
    GH_CHECK_HIP(ctx, hipGetLastError());
    return GRIDHIP_OK;
}

namespace {

// the conjugate of an n-element complex table, in a block of the pool
int conj_copy(gridhip_ctx *ctx, DevBuf &b, int64_t n, const double *in, const double **out)
{
    GH_CHECK(b.alloc(ctx, (size_t)n * 16));
    hipLaunchKernelGGL(conj_copy_kernel, grid_for(ctx, n), dim3(256), 0, ctx->stream, n, (const double2 *)in,
                       b.as<double2>());
    GH_CHECK_HIP(ctx, hipGetLastError());
    *out = b.as<double>();
    return GRIDHIP_OK;
}

// F = fft_c(model) into f (N x N complex); t: N x N complex scratch for odd N
int model_transform(gridhip_ctx *ctx, int64_t N, const double *model, DevBuf &f, DevBuf &t)
{
    const size_t cells = (size_t)N * N;
    GH_CHECK(f.alloc(ctx, cells * 16));
    if (N % 2 != 0) GH_CHECK(t.alloc(ctx, cells * 16));
    return model_transform_to(ctx, N, model, f.as<double2>(), t.as<double2>(), nullptr);
}

struct PredictArgs {
    ImagingFn fn;
    const double *model;
    int64_t n;
    const double *u, *v, *w;
    int64_t stride;
    const double *vis_sub;
    double *vis_out;
};

// Everything is checked before anything is touched: a refused call leaves vis_out as it was.
int predict_check(gridhip_ctx *ctx, PredictArgs &a, int64_t *N)
{
    GH_CHECK(imaging_fn_check(ctx, a.fn, N));
    if (!a.model || a.n < 0 || a.stride < 1 || (a.n > 0 && (!a.u || !a.v || !a.vis_out || (a.fn.kind == 2 && !a.w))))
        return fail(ctx, GRIDHIP_EINVAL, "bad argument");
    if (a.n > (int64_t)0x7fffff00) return fail(ctx, GRIDHIP_EUNSUPPORTED, "n must be < 2^31 per call");
    return GRIDHIP_OK;
}

// timing events (gridhip_timing): 0 before the transform, 1 after it, 2 after the gather and the epilogue; the
// gathers' own events are switched off meanwhile
struct NoTiming {
    gridhip_ctx *ctx;
    bool was;
    explicit NoTiming(gridhip_ctx *c) : ctx(c), was(c->timing) { c->timing = false; }
    ~NoTiming() { ctx->timing = was; }
};

// vis_out (device) = pred or vis_sub - pred
int predict_tail(gridhip_ctx *ctx, int64_t n, const DevBuf &pred, const double *vis_sub, double *vis_out)
{
    hipLaunchKernelGGL(residual_kernel, grid_for(ctx, n), dim3(256), 0, ctx->stream, n, (const double2 *)pred.p,
                       (const double2 *)vis_sub, (double2 *)vis_out);
    GH_CHECK_HIP(ctx, hipGetLastError());
    mark(ctx, 2);
    return GRIDHIP_OK;
}

int predict_any(gridhip_ctx *ctx, bool dev, PredictArgs a)
{
    if (!ctx) return GRIDHIP_EINVAL;
    int64_t N = 0;
    GH_CHECK(predict_check(ctx, a, &N));
    const ImagingFn &fn = a.fn;
    GH_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    const int64_t n = a.n;
    // nothing is dropped until a gather says otherwise (the simple gather counts nothing, as `grid` does not)
    GH_CHECK_HIP(ctx, hipMemsetAsync(ctx->d_scalars, 0, 4 * sizeof(int32_t), ctx->stream));
    Staged st(ctx, dev);
    if (n == 0) return st.finish();
    const size_t cells = (size_t)N * N, span = span_bytes(n, a.stride);
    // the arguments on the device (w and kv: for the kind that reads them)
    const double *model = st.in(a.model, cells * 8), *u = st.in(a.u, span), *v = st.in(a.v, span);
    const double *w = fn.kind == 2 ? st.in(a.w, span) : nullptr;
    const double *kv = fn.kind == 1 ? st.in(fn.kv, (size_t)fn.Q * fn.Q * fn.gh * fn.gw * 16) : nullptr;
    const double *vis_sub = st.in(a.vis_sub, (size_t)n * 16);
    double *out = st.out(a.vis_out, (size_t)n * 16);
    GH_CHECK(st.status());
    // front end: the imaging function's coordinates (p = uvw / lam; w_cache: the w-bins and its kernel table)
    DevBuf pu, pv, pw;
    WCache wc;
    if (fn.kind == 1) {
        GH_CHECK(scaled_uv(ctx, n, u, v, a.stride, (double)fn.lam, pu, pv));
    } else if (fn.kind == 2) {
        if (a.stride != 1) {  // (w_cache_prepare takes contiguous columns: slice the (n, 3) matrix)
            GH_CHECK(slice_uvw(ctx, n, u, v, w, a.stride, pu, pv, pw));
            u = pu.as<double>(), v = pv.as<double>(), w = pw.as<double>();
        }
        GH_CHECK(w_cache_prepare(ctx, wc, fn.theta, fn.lam, fn.wstep, fn.Q, fn.npixFF, fn.gh, n, u, v, w));
    }
    DevBuf f, t, pred, ctab;
    GH_CHECK(pred.alloc(ctx, (size_t)n * 16));
    mark(ctx, 0);
    GH_CHECK(model_transform(ctx, N, model, f, t));
    mark(ctx, 1);
    {
        NoTiming quiet(ctx);
        if (fn.kind == 0) {
            GH_CHECK(launch_simple_degrid(ctx, N, N, f.as<const double2>(), n, u, v, a.stride, (double)fn.lam,
                                          pred.as<double2>()));
        } else if (fn.kind == 1) {
            const double *k = nullptr;
            GH_CHECK(conj_copy(ctx, ctab, fn.Q * fn.Q * fn.gh * fn.gw, kv, &k));
            GH_CHECK(gridhip_degrid2_dev(ctx, N, N, f.as<double>(), n, 1, fn.Q, fn.gh, fn.gw, k, pu.as<double>(),
                                         pv.as<double>(), 1, nullptr, pred.as<double>()));
        } else {
            // the cached table holds conj(w_kernel) per plane (w_cache_imaging's); the gather wants w_kernel
            const double *k = nullptr;
            GH_CHECK(conj_copy(ctx, ctab, wc.nplanes * fn.Q * fn.Q * fn.gh * fn.gh, (const double *)wc.table, &k));
            GH_CHECK(gridhip_degrid2_dev(ctx, N, N, f.as<double>(), n, wc.nplanes, fn.Q, fn.gh, fn.gh, k,
                                         wc.pu.as<double>(), wc.pv.as<double>(), 1, wc.wb.as<int64_t>(),
                                         pred.as<double>()));
        }
    }
    GH_CHECK(predict_tail(ctx, n, pred, vis_sub, out));
    return st.finish();
}

int predict_aw_any(gridhip_ctx *ctx, bool dev, const AwArgs &a, const double *model, const double *vis_sub,
                   double *vis_out)
{
    if (!ctx) return GRIDHIP_EINVAL;
    int64_t N = 0;
    GH_CHECK(aw_check(ctx, a, &N, false));
    if (!model || (a.n > 0 && !vis_out)) return fail(ctx, GRIDHIP_EINVAL, "bad argument");
    GH_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    const int64_t n = a.n;
    GH_CHECK_HIP(ctx, hipMemsetAsync(ctx->d_scalars, 0, 4 * sizeof(int32_t), ctx->stream));
    Staged st(ctx, dev);
    if (n == 0) return st.finish();
    const AwArgs d = stage_aw(st, a);
    model = st.in(model, (size_t)N * N * 8), vis_sub = st.in(vis_sub, (size_t)n * 16);
    vis_out = st.out(vis_out, (size_t)n * 16);
    GH_CHECK(st.status());
    AwFront fr;
    GH_CHECK(aw_front(ctx, N, d, 1.0, false, 0, false, fr));  // p = uvw / lam, findClosest w-bins; no mirror
    DevBuf f, t, pred, cwk, cak;
    GH_CHECK(pred.alloc(ctx, (size_t)n * 16));
    mark(ctx, 0);
    GH_CHECK(model_transform(ctx, N, model, f, t));
    mark(ctx, 1);
    {
        NoTiming quiet(ctx);
        // awdegrid gathers with conj(aw_kernel_fn2(its wkerns, akerns)); aw_imaging grids with conj(aw_kernel_fn2(wk,
        // ak)), whose adjoint gathers with aw_kernel_fn2(wk, ak) = conj(aw_kernel_fn2(conj wk, conj ak))
        const double *wk = nullptr, *ak = nullptr;
        GH_CHECK(conj_copy(ctx, cwk, d.W * d.Q * d.Q * d.S * d.S, d.wkerns, &wk));
        GH_CHECK(conj_copy(ctx, cak, d.A * d.S * d.S, d.akerns, &ak));
        GH_CHECK(gridhip_awdegrid_dev(ctx, N, N, f.as<double>(), n, d.W, d.Q, d.S, d.A, wk, ak, fr.pu.as<double>(),
                                      fr.pv.as<double>(), 1, fr.wb.as<int64_t>(), d.a1, d.a2, pred.as<double>()));
    }
    GH_CHECK(predict_tail(ctx, n, pred, vis_sub, vis_out));
    return st.finish();
}

}  // namespace
}  // namespace gridhip

using namespace gridhip;

extern "C" {

int gridhip_predict(gridhip_ctx *ctx, int kind, int64_t wstep, int64_t Q, int64_t npixFF, int64_t gh, int64_t gw,
                    const double *kv, double theta, int64_t lam, const double *model, int64_t n, const double *u,
                    const double *v, const double *w, int64_t uv_stride, const double *vis_sub, double *vis_out)
{
    return predict_any(ctx, false, {{kind, wstep, Q, npixFF, gh, gw, kv, theta, lam}, model, n, u, v, w, uv_stride, vis_sub,
                                    vis_out});
}

int gridhip_predict_dev(gridhip_ctx *ctx, int kind, int64_t wstep, int64_t Q, int64_t npixFF, int64_t gh, int64_t gw,
                        const double *kv, double theta, int64_t lam, const double *model, int64_t n, const double *u,
                        const double *v, const double *w, int64_t uv_stride, const double *vis_sub, double *vis_out)
{
    return predict_any(ctx, true, {{kind, wstep, Q, npixFF, gh, gw, kv, theta, lam}, model, n, u, v, w, uv_stride, vis_sub,
                                   vis_out});
}

int gridhip_predict_aw(gridhip_ctx *ctx, double theta, int64_t lam, int64_t W, int64_t Q, int64_t S, int64_t A,
                       const double *wkerns, const double *wvals, const double *akerns, const double *model, int64_t n,
                       const double *u, const double *v, const double *w, int64_t uv_stride, const int64_t *a1,
                       const int64_t *a2, const double *vis_sub, double *vis_out)
{
    const AwArgs a{theta, lam, W, Q, S, A, wkerns, wvals, akerns, n, u, v, w, uv_stride, a1, a2, nullptr};
    return predict_aw_any(ctx, false, a, model, vis_sub, vis_out);
}

int gridhip_predict_aw_dev(gridhip_ctx *ctx, double theta, int64_t lam, int64_t W, int64_t Q, int64_t S, int64_t A,
                           const double *wkerns, const double *wvals, const double *akerns, const double *model,
                           int64_t n, const double *u, const double *v, const double *w, int64_t uv_stride,
                           const int64_t *a1, const int64_t *a2, const double *vis_sub, double *vis_out)
{
    const AwArgs a{theta, lam, W, Q, S, A, wkerns, wvals, akerns, n, u, v, w, uv_stride, a1, a2, nullptr};
    return predict_aw_any(ctx, true, a, model, vis_sub, vis_out);
}

}  // extern "C"
