// The imaging functions (simple, conv, w_cache, aw) and do_imaging, which strings the operations of image_ops.hip and
// the gridders together (src/Gridding.hs:84-124, 399-549; src/ImageDataset.hs:54-77).
#include "common.h"
#include "imaging.h"

namespace gridhip {

int imaging_fn_check(gridhip_ctx *ctx, ImagingFn &fn, int64_t *N)
{
    *N = gridhip_image_size(fn.theta, fn.lam);
    if (fn.kind == 2 && fn.wstep <= 0) fn.wstep = 2000;  // (w_cache_imaging's default, :412)
    const bool ok = fn.kind == 0 || (fn.kind == 1 && fn.kv && fn.Q > 0 && fn.gh > 0 && fn.gw > 0) ||
                    (fn.kind == 2 && w_kernel_shape_ok(fn.npixFF, fn.gh, fn.Q));
    if (*N <= 0 || !ok)
        return fail(ctx, GRIDHIP_EINVAL, "bad imaging function %d, its options (kind 2: the w-kernel shape rule), or image size %lld",
                    fn.kind, (long long)*N);
    return GRIDHIP_OK;
}

// Front end of the aw entry points, kernel 1 of 2: one read of the strided (u, v, w) and vis per visibility.
//   uvw_lambda (ImageDataset.hs:181-187: x fc = f / c; fc = 1 for uvw already in wavelengths - an exact product),
//   mirror_uvw (Gridding.hs:551-562: v < 0 negates u, v, w and conjugates vis; the antennas are NOT swapped),
//   p = uvw1 / lam and the findClosest w-bin of w1 in wavelengths (aw_imaging, :466-474),
//   doweight's cell (:564-583) of the mirrored coordinates (weigh 1: do_imaging, :531-535) or of the un-mirrored ones
//   (weigh 2: aw_gridding, ImageDataset.hs:59-60), counted into the histogram.  The cell is stored, not re-derived
//   by kernel 2 from p: floor(0.5 + x) is not odd-symmetric, so the two coordinate sets can give different cells.
// vis1 may be NULL when nothing is mirrored (aw_imaging: the caller's vis is gridded as it is).
__global__ void aw_front_kernel(int64_t n, const double *__restrict__ u, const double *__restrict__ v,
                                const double *__restrict__ w, int64_t stride, const double2 *__restrict__ vis, double fc,
                                double lam, int mirror, int weigh, int64_t N, int64_t nws, const double *__restrict__ ws,
                                double *__restrict__ pu, double *__restrict__ pv, int64_t *__restrict__ wbin,
                                double2 *__restrict__ vis1, int64_t *__restrict__ cell, unsigned int *__restrict__ cnt)
{
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x) {
        const double u0 = u[k * stride] * fc, v0 = v[k * stride] * fc, w0 = w[k * stride] * fc;
        const bool neg = mirror && v0 < 0;
        const double u1 = neg ? -u0 : u0, v1 = neg ? -v0 : v0, w1 = neg ? -w0 : w0;
        const double qu = u1 / lam, qv = v1 / lam;
        pu[k] = qu;
        pv[k] = qv;
        wbin[k] = closest_index(nws, ws, w1);
        if (vis1) {
            double2 x = vis[k];
            if (neg) x.y = -x.y;
            vis1[k] = x;
        }
        if (weigh) {
            const int64_t c = weigh == 1 ? weight_cell(N, qu, qv) : weight_cell(N, u0 / lam, v0 / lam);
            cell[k] = c;
            if (c >= 0) atomicAdd(&cnt[c], 1u);
        }
    }
}

// kernel 2 of 2: wt = doweight's ones / count (the same two divisions as weight_apply_kernel; a visibility outside the
// grid keeps 1) and, in place, vis1 = wt * vis1 (the product of cmul_real_kernel).  wt may be NULL (aw_gridding).
__global__ void aw_weight_kernel(int64_t n, const int64_t *__restrict__ cell, const unsigned int *__restrict__ cnt,
                                 double2 *vis1, double2 *__restrict__ wt)
{
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x) {
        double2 a = make_double2(1.0, 0.0);
        const int64_t c = cell[k];
        if (c >= 0) {
            const double wgt = (double)cnt[c];
            a.x /= wgt;
            a.y /= wgt;
        }
        const double2 y = vis1[k];
        if (wt) wt[k] = a;
        vis1[k] = make_double2(a.x * y.x - a.y * y.y, a.x * y.y + a.y * y.x);
    }
}

__global__ void cmul_real_kernel(int64_t n, const double2 *__restrict__ a, const double2 *__restrict__ b,
                                 double2 *__restrict__ out)
{
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x) {
        const double2 x = a[k], y = b[k];
        out[k] = make_double2(x.x * y.x - x.y * y.y, x.x * y.y + x.y * y.x);
    }
}

__global__ void fill_ones_kernel(int64_t n, double2 *__restrict__ a)
{
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x)
        a[k] = make_double2(1.0, 0.0);
}

// what do_imaging's weighting needs beside launch_doweight: a = 1 + 0i, and out = a * b (both on ctx->stream)
int launch_fill_ones(gridhip_ctx *ctx, int64_t n, double2 *a)
{
    if (n > 0) hipLaunchKernelGGL(fill_ones_kernel, grid_for(ctx, n), dim3(256), 0, ctx->stream, n, a);
    GH_CHECK_HIP(ctx, hipGetLastError());
    return GRIDHIP_OK;
}

int launch_cmul(gridhip_ctx *ctx, int64_t n, const double2 *a, const double2 *b, double2 *out)
{
    if (n > 0) hipLaunchKernelGGL(cmul_real_kernel, grid_for(ctx, n), dim3(256), 0, ctx->stream, n, a, b, out);
    GH_CHECK_HIP(ctx, hipGetLastError());
    return GRIDHIP_OK;
}

// mirror + weights + the two gridding passes + hermitian + iFFT + normalise, all on the device.
// `imgfn` grids (u1, v1, w1, vis) -> zeroed N x N grid.  st: the call's staging, which may hold arguments of the
// caller's already (conv_imaging's kv); the array arguments here are the caller's own, taken through it.
template <typename ImgFn>
static int do_imaging_impl(gridhip_ctx *ctx, Staged &st, int64_t N, int64_t lam, int64_t n, const double *u,
                           const double *v, const double *w, int64_t stride, const double *vis, double *image,
                           double *psf, double *pmax, ImgFn imgfn)
{
    const size_t cells = (size_t)N * N, span = span_bytes(n, stride);
    u = st.in(u, span), v = st.in(v, span), w = st.in(w, span), vis = st.in(vis, n * 16);
    image = st.out(image, cells * 8), psf = st.out(psf, cells * 8);
    GH_CHECK(st.status());
    DevBuf du, dv, dw, dvis, dwt, dpu, dpv, dg, dh, dtmp, dreal, dmax;
    GH_CHECK(dvis.alloc(ctx, n * 16));
    GH_CHECK(dwt.alloc(ctx, n * 16));
    GH_CHECK(dg.alloc(ctx, cells * 16));
    GH_CHECK(dh.alloc(ctx, cells * 16));
    GH_CHECK(dtmp.alloc(ctx, cells * 16));
    GH_CHECK(dreal.alloc(ctx, cells * 8));
    GH_CHECK(dmax.alloc(ctx, 8));
    // slice the columns (src/Gridding.hs:524-526)
    GH_CHECK(slice_uvw(ctx, n, u, v, w, stride, du, dv, dw));
    // mirror baselines such that v >= 0 (:531): in place, so on a copy of vis
    GH_CHECK(copy_in(ctx, dvis.p, vis, n * 16, true));
    GH_CHECK(launch_mirror(ctx, n, du.as<double>(), dv.as<double>(), dw.as<double>(), dvis.as<double2>()));
    // weights (:534-535): doweight theta lam uvw1 ones
    GH_CHECK(scaled_uv(ctx, n, du.as<double>(), dv.as<double>(), 1, (double)lam, dpu, dpv));
    if (n > 0) {
        hipLaunchKernelGGL(fill_ones_kernel, grid_for(ctx, n), dim3(256), 0, ctx->stream, n, dwt.as<double2>());
        GH_CHECK_HIP(ctx, hipMemsetAsync(dtmp.p, 0, cells * 4, ctx->stream));
        GH_CHECK(launch_doweight(ctx, N, n, dpu.as<double>(), dpv.as<double>(), dtmp.as<unsigned int>(), dwt.as<double2>()));
        // wt * vis1 (:538)
        hipLaunchKernelGGL(cmul_real_kernel, grid_for(ctx, n), dim3(256), 0, ctx->stream, n, dwt.as<double2>(),
                           dvis.as<double2>(), dvis.as<double2>());
    }
    for (int pass = 0; pass < 2; ++pass) {
        // pass 0: image from wt*vis (:538-539) into dreal; pass 1: PSF from wt (:541-542) into dtmp, and its maximum
        GH_CHECK_HIP(ctx, hipMemsetAsync(dg.p, 0, cells * 16, ctx->stream));
        GH_CHECK(imgfn(du.as<double>(), dv.as<double>(), dw.as<double>(), pass == 0 ? dvis.as<double>() : dwt.as<double>(),
                       dg.as<double>()));
        GH_CHECK(image_tail(ctx, N, dg.as<double2>(), dh.as<double2>(), pass == 0 ? dreal.as<double>() : dtmp.as<double>(),
                            pass == 1 ? dmax.as<unsigned long long>() : nullptr));
    }
    GH_CHECK(normalise(ctx, cells, dreal.as<double>(), dtmp.as<double>(), dmax.as<unsigned long long>(), pmax));
    if (image) GH_CHECK(copy_out(ctx, image, dreal.p, cells * 8, true));
    if (psf) GH_CHECK(copy_out(ctx, psf, dtmp.p, cells * 8, true));
    GH_CHECK(st.finish());
    return sync(ctx);  // (the device-resident form, too, returns with image and psf written)
}

// (WCache: imaging.h)
int w_cache_prepare(gridhip_ctx *ctx, WCache &c, double theta, int64_t lam, int64_t wstep, int64_t Q,
                           int64_t npixFF, int64_t S, int64_t n, const double *u, const double *v, const double *w)
{
    GH_CHECK(scaled_uv(ctx, n, u, v, 1, (double)lam, c.pu, c.pv));
    GH_CHECK(c.wb.alloc(ctx, n * 8));
    int64_t wmin = 0;
    GH_CHECK(dev_wbins(ctx, n, w, 1, wstep, c.wb.as<int64_t>(), &wmin, &c.nplanes));
    c.ready = true;
    if (n == 0 || c.nplanes == 0) return GRIDHIP_OK;
    if (c.nplanes > 65536) return fail(ctx, GRIDHIP_EUNSUPPORTED, "%lld w-planes", (long long)c.nplanes);
    auto &k = ctx->img->wk_cache;
    const size_t bytes = (size_t)c.nplanes * Q * Q * S * S * 16;
    if (!(k.ptr && k.theta == theta && k.wstep == wstep && k.wmin == wmin && k.nplanes == c.nplanes && k.npixFF == npixFF &&
          k.S == S && k.Q == Q)) {
        k.nplanes = 0;  // (not valid while it is rebuilt)
        if (k.bytes < bytes) {
            if (k.ptr) {
                GH_CHECK(sync(ctx));  // (the old table may still be read by work queued on the stream)
                (void)hipFree(k.ptr);
                k.ptr = nullptr;
                k.bytes = 0;
            }
            if (hipMalloc(&k.ptr, bytes) != hipSuccess) {
                k.ptr = nullptr;
                return fail(ctx, GRIDHIP_ENOMEM, "w-kernel table: %zu bytes", bytes);
            }
            k.bytes = bytes;
            GH_CHECK(scratch_prefill(ctx, k.ptr, bytes));
        }
        GH_CHECK(build_w_planes(ctx, theta, wstep, wmin, c.nplanes, npixFF, S, Q, (double2 *)k.ptr, true));  // (:441)
        GH_CHECK(sync(ctx));
        k.theta = theta;
        k.wstep = wstep;
        k.wmin = wmin;
        k.nplanes = c.nplanes;
        k.npixFF = npixFF;
        k.S = S;
        k.Q = Q;
    }
    c.table = (double2 *)k.ptr;
    return GRIDHIP_OK;
}

// u,v,w in wavelengths, grid zeroed N x N
static int w_cache_grid_dev(gridhip_ctx *ctx, WCache &c, double theta, int64_t lam, int64_t wstep, int64_t Q,
                            int64_t npixFF, int64_t S, int64_t N, int64_t n, const double *u, const double *v,
                            const double *w, const double *vis, double *grid)
{
    if (!c.ready) GH_CHECK(w_cache_prepare(ctx, c, theta, lam, wstep, Q, npixFF, S, n, u, v, w));
    if (n == 0 || c.nplanes == 0) return GRIDHIP_OK;
    if (!c.plan)
        GH_CHECK(plan_create_borrowed(ctx, N, N, n, c.nplanes, Q, S, S, c.pu.as<double>(), c.pv.as<double>(), 1,
                                      c.wb.as<int64_t>(), &c.plan));  // (nothing else grids on this context before both passes are done)
    GH_CHECK(gridhip_plan_grid_dev(c.plan, (const double *)c.table, vis, grid));
    return sync(ctx);
}

// ---- the aw entry points (aw_imaging_dev, do_imaging_aw, aw_gridding): front end -> aw gridder -> imaging tail ----

// (AwArgs: imaging.h)
// Everything is checked before anything is touched (a refused call leaves its outputs as they were).
int aw_check(gridhip_ctx *ctx, const AwArgs &a, int64_t *N, bool vis_needed)
{
    *N = gridhip_image_size(a.theta, a.lam);
    if (*N <= 0 || a.n < 0 || a.stride < 1 || a.W <= 0 || a.Q <= 0 || a.S <= 0 || a.A <= 0 || !a.wkerns || !a.wvals ||
        !a.akerns || (a.n > 0 && (!a.u || !a.v || !a.w || !a.a1 || !a.a2 || (vis_needed && !a.vis))))
        return fail(ctx, GRIDHIP_EINVAL, "bad argument");
    if (ctx->opt.aw_batch < 0) return fail(ctx, GRIDHIP_EINVAL, "option 'aw_batch' must be >= 0");
    return GRIDHIP_OK;
}

AwArgs stage_aw(Staged &st, const AwArgs &a)
{
    const size_t span = span_bytes(a.n, a.stride);
    AwArgs d = a;
    d.wkerns = st.in(a.wkerns, (size_t)a.W * a.Q * a.Q * a.S * a.S * 16);
    d.wvals = st.in(a.wvals, (size_t)a.W * 8);
    d.akerns = st.in(a.akerns, (size_t)a.A * a.S * a.S * 16);
    d.u = st.in(a.u, span), d.v = st.in(a.v, span), d.w = st.in(a.w, span);
    d.a1 = st.in(a.a1, (size_t)a.n * 8), d.a2 = st.in(a.a2, (size_t)a.n * 8);
    d.vis = st.in(a.vis, (size_t)a.n * 16);  // (predict_aw reads no vis: null)
    return d;
}

// (AwFront: imaging.h)
int aw_front(gridhip_ctx *ctx, int64_t N, const AwArgs &d, double fc, bool mirror, int weigh, bool want_wt,
                    AwFront &f)
{
    const int64_t n = d.n;
    GH_CHECK(f.pu.alloc(ctx, n * 8));
    GH_CHECK(f.pv.alloc(ctx, n * 8));
    GH_CHECK(f.wb.alloc(ctx, n * 8));
    if (mirror) GH_CHECK(f.vis1.alloc(ctx, n * 16));
    if (want_wt) GH_CHECK(f.wt.alloc(ctx, n * 16));
    if (weigh) {
        GH_CHECK(f.cell.alloc(ctx, n * 8));
        GH_CHECK(f.cnt.alloc(ctx, (size_t)N * N * 4));
        GH_CHECK_HIP(ctx, hipMemsetAsync(f.cnt.p, 0, (size_t)N * N * 4, ctx->stream));
    }
    if (n > 0) {
        hipLaunchKernelGGL(aw_front_kernel, grid_for(ctx, n), dim3(256), 0, ctx->stream, n, d.u, d.v, d.w, d.stride,
                           (const double2 *)d.vis, fc, (double)d.lam, mirror ? 1 : 0, weigh, N, d.W, d.wvals,
                           f.pu.as<double>(), f.pv.as<double>(), f.wb.as<int64_t>(),
                           mirror ? f.vis1.as<double2>() : (double2 *)nullptr,
                           weigh ? f.cell.as<int64_t>() : (int64_t *)nullptr,
                           weigh ? f.cnt.as<unsigned int>() : (unsigned int *)nullptr);
        if (weigh)
            hipLaunchKernelGGL(aw_weight_kernel, grid_for(ctx, n), dim3(256), 0, ctx->stream, n, f.cell.as<int64_t>(),
                               f.cnt.as<unsigned int>(), f.vis1.as<double2>(),
                               want_wt ? f.wt.as<double2>() : (double2 *)nullptr);
    }
    GH_CHECK_HIP(ctx, hipGetLastError());
    return GRIDHIP_OK;
}

// aw_imaging on device-resident arguments d: the front end's one kernel (p = uvw / lam, findClosest w-bins; NB the
// reference searches with w in wavelengths, not w / lam, :473-474), then the aw gridder into the N x N grid (zeroed
// first).  Asynchronous.
static int aw_imaging_to(gridhip_ctx *ctx, int64_t N, const AwArgs &d, double *grid)
{
    GH_CHECK_HIP(ctx, hipMemsetAsync(grid, 0, (size_t)N * N * 16, ctx->stream));
    AwFront f;
    GH_CHECK(aw_front(ctx, N, d, 1.0, false, 0, false, f));
    return awgrid_pairs(ctx, N, N, 1, &grid, &d.vis, d.n, d.W, d.Q, d.S, d.A, d.wkerns, d.akerns, f.pu.as<double>(),
                        f.pv.as<double>(), 1, f.wb.as<int64_t>(), d.a1, d.a2);
}

// do_imaging with imgfn = aw_imaging (src/Gridding.hs:509-549): doweight on the MIRRORED uvw (:531-535); both gridding
// passes in one aw batch loop (one kernel table per batch), then two tails and the normalisation.
static int do_imaging_aw_any(gridhip_ctx *ctx, bool dev, const AwArgs &a, double *image, double *psf, double *pmax)
{
    if (!ctx) return GRIDHIP_EINVAL;
    int64_t N = 0;
    GH_CHECK(aw_check(ctx, a, &N));
    if (!image || !psf) return fail(ctx, GRIDHIP_EINVAL, "bad argument");
    GH_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    const size_t cells = (size_t)N * N;
    Staged st(ctx, dev);
    const AwArgs d = stage_aw(st, a);
    image = st.out(image, cells * 8), psf = st.out(psf, cells * 8);
    GH_CHECK(st.status());
    AwFront f;
    GH_CHECK(aw_front(ctx, N, d, 1.0, true, 1, true, f));
    // both grids are filled by the one batch loop before either is transformed: two N x N complex blocks
    DevBuf dg0, dg1, dh, dmax;
    GH_CHECK(dg0.alloc(ctx, cells * 16));
    GH_CHECK(dg1.alloc(ctx, cells * 16));
    GH_CHECK(dh.alloc(ctx, cells * 16));
    GH_CHECK(dmax.alloc(ctx, 8));
    GH_CHECK_HIP(ctx, hipMemsetAsync(dg0.p, 0, cells * 16, ctx->stream));
    GH_CHECK_HIP(ctx, hipMemsetAsync(dg1.p, 0, cells * 16, ctx->stream));
    double *grids[2] = {dg0.as<double>(), dg1.as<double>()};
    const double *viss[2] = {f.vis1.as<double>(), f.wt.as<double>()};  // image from wt * vis1 (:538), PSF from wt (:541)
    GH_CHECK(awgrid_pairs(ctx, N, N, 2, grids, viss, d.n, d.W, d.Q, d.S, d.A, d.wkerns, d.akerns, f.pu.as<double>(),
                          f.pv.as<double>(), 1, f.wb.as<int64_t>(), d.a1, d.a2));
    GH_CHECK(image_tail(ctx, N, dg0.as<double2>(), dh.as<double2>(), image, nullptr));
    GH_CHECK(image_tail(ctx, N, dg1.as<double2>(), dh.as<double2>(), psf, dmax.as<unsigned long long>()));
    GH_CHECK(normalise(ctx, cells, image, psf, dmax.as<unsigned long long>(), pmax));
    return st.finish();
}

// aw_gridding, src/ImageDataset.hs:54-77: uvw in metres -> uvw_lambda (x f / c) -> doweight on the UN-mirrored uvw
// (:59) -> mirror_uvw (:60) -> aw_imaging of vis1 * wt (:72-73) -> make_grid_hermitian -> real . ifft, and its maximum.
static int aw_gridding_any(gridhip_ctx *ctx, bool dev, const AwArgs &a, double f, double *image, double *imax)
{
    if (!ctx) return GRIDHIP_EINVAL;
    int64_t N = 0;
    GH_CHECK(aw_check(ctx, a, &N));
    if (!image || !(f > 0.0) || !(f < INFINITY)) return fail(ctx, GRIDHIP_EINVAL, "bad argument");
    GH_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    const size_t cells = (size_t)N * N;
    Staged st(ctx, dev);
    const AwArgs d = stage_aw(st, a);
    image = st.out(image, cells * 8);
    GH_CHECK(st.status());
    AwFront fr;
    GH_CHECK(aw_front(ctx, N, d, f / 299792458.0, true, 2, false, fr));  // (the constant of uvw_lambda, :187)
    DevBuf dg, dh, dmax;
    GH_CHECK(dg.alloc(ctx, cells * 16));
    GH_CHECK(dh.alloc(ctx, cells * 16));
    GH_CHECK(dmax.alloc(ctx, 8));
    GH_CHECK_HIP(ctx, hipMemsetAsync(dg.p, 0, cells * 16, ctx->stream));
    double *grid = dg.as<double>();
    const double *vis = fr.vis1.as<double>();
    GH_CHECK(awgrid_pairs(ctx, N, N, 1, &grid, &vis, d.n, d.W, d.Q, d.S, d.A, d.wkerns, d.akerns, fr.pu.as<double>(),
                          fr.pv.as<double>(), 1, fr.wb.as<int64_t>(), d.a1, d.a2));
    GH_CHECK(image_tail(ctx, N, dg.as<double2>(), dh.as<double2>(), image, dmax.as<unsigned long long>()));
    unsigned long long mb = 0;
    GH_CHECK(d2h(ctx, &mb, dmax.p, 8));
    GH_CHECK(sync(ctx));
    if (imax) *imax = ordered_value(mb);
    return st.finish();
}

}  // namespace gridhip

using namespace gridhip;

extern "C" {

// ---- imaging functions (ImagingFunction, src/Gridding.hs:76-81): uvw in wavelengths, returns the N x N grid ----

static int simple_grid_dev(gridhip_ctx *ctx, int64_t lam, int64_t N, int64_t n, const double *u, const double *v,
                           const double *vis, double *grid)
{
    DevBuf pu, pv;
    GH_CHECK(scaled_uv(ctx, n, u, v, 1, (double)lam, pu, pv));
    GH_CHECK(gridhip_grid_dev(ctx, N, N, grid, n, pu.as<double>(), pv.as<double>(), 1, vis));
    return sync(ctx);
}

static int conv_grid_dev(gridhip_ctx *ctx, int64_t lam, int64_t N, int64_t Q, int64_t gh, int64_t gw,
                         const double *dkv, int64_t n, const double *u, const double *v, const double *vis,
                         double *grid)
{
    DevBuf pu, pv;
    GH_CHECK(scaled_uv(ctx, n, u, v, 1, (double)lam, pu, pv));
    GH_CHECK(gridhip_convgrid_dev(ctx, N, N, grid, n, Q, gh, gw, dkv, pu.as<double>(), pv.as<double>(), 1, vis));
    return sync(ctx);
}

// simple_imaging, src/Gridding.hs:84-93
int gridhip_simple_imaging(gridhip_ctx *ctx, double theta, int64_t lam, int64_t n, const double *u, const double *v,
                           int64_t uv_stride, const double *vis, double *grid)
{
    if (!ctx) return GRIDHIP_EINVAL;
    const int64_t N = gridhip_image_size(theta, lam);
    if (N <= 0 || n < 0 || uv_stride < 1 || !grid || (n > 0 && (!u || !v || !vis)))
        return fail(ctx, GRIDHIP_EINVAL, "bad argument");
    GH_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    Staged st(ctx, false);
    u = st.in(u, span_bytes(n, uv_stride)), v = st.in(v, span_bytes(n, uv_stride)), vis = st.in(vis, (size_t)n * 16);
    grid = st.out(grid, (size_t)N * N * 16);
    GH_CHECK(st.status());
    DevBuf du, dv, dw;
    GH_CHECK(slice_uvw(ctx, n, u, v, nullptr, uv_stride, du, dv, dw));
    GH_CHECK_HIP(ctx, hipMemsetAsync(grid, 0, (size_t)N * N * 16, ctx->stream));
    GH_CHECK(simple_grid_dev(ctx, lam, N, n, du.as<double>(), dv.as<double>(), vis, grid));
    return st.finish();
}

// conv_imaging kv, src/Gridding.hs:115-124 ; kv is [Q][Q][gh][gw]
int gridhip_conv_imaging(gridhip_ctx *ctx, int64_t Q, int64_t gh, int64_t gw, const double *kv, double theta,
                         int64_t lam, int64_t n, const double *u, const double *v, int64_t uv_stride,
                         const double *vis, double *grid)
{
    if (!ctx) return GRIDHIP_EINVAL;
    const int64_t N = gridhip_image_size(theta, lam);
    if (N <= 0 || n < 0 || uv_stride < 1 || !grid || !kv || Q <= 0 || gh <= 0 || gw <= 0 ||
        (n > 0 && (!u || !v || !vis)))
        return fail(ctx, GRIDHIP_EINVAL, "bad argument");
    GH_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    Staged st(ctx, false);
    u = st.in(u, span_bytes(n, uv_stride)), v = st.in(v, span_bytes(n, uv_stride)), vis = st.in(vis, (size_t)n * 16);
    kv = st.in(kv, (size_t)Q * Q * gh * gw * 16), grid = st.out(grid, (size_t)N * N * 16);
    GH_CHECK(st.status());
    DevBuf du, dv, dw;
    GH_CHECK(slice_uvw(ctx, n, u, v, nullptr, uv_stride, du, dv, dw));
    GH_CHECK_HIP(ctx, hipMemsetAsync(grid, 0, (size_t)N * N * 16, ctx->stream));
    GH_CHECK(conv_grid_dev(ctx, lam, N, Q, gh, gw, kv, n, du.as<double>(), dv.as<double>(), vis, grid));
    return st.finish();
}

// w_cache_imaging, src/Gridding.hs:399-449 (wstep default 2000, :412): uvw in wavelengths, the N x N grid overwritten
static int w_cache_imaging_any(gridhip_ctx *ctx, bool dev, int64_t wstep, int64_t qpx, int64_t npixFF, int64_t npixKern,
                               double theta, int64_t lam, int64_t n, const double *u, const double *v, const double *w,
                               int64_t uv_stride, const double *vis, double *grid)
{
    if (!ctx) return GRIDHIP_EINVAL;
    ImagingFn fn{2, wstep, qpx, npixFF, npixKern, npixKern, nullptr, theta, lam};
    int64_t N = 0;
    GH_CHECK(imaging_fn_check(ctx, fn, &N));
    if (n < 0 || uv_stride < 1 || !grid || (n > 0 && (!u || !v || !w || !vis))) return fail(ctx, GRIDHIP_EINVAL, "bad argument");
    GH_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    const size_t span = span_bytes(n, uv_stride);
    Staged st(ctx, dev);
    u = st.in(u, span), v = st.in(v, span), w = st.in(w, span), vis = st.in(vis, (size_t)n * 16);
    grid = st.out(grid, (size_t)N * N * 16);
    GH_CHECK(st.status());
    DevBuf du, dv, dw;
    if (uv_stride != 1) {  // the (n, 3) matrix: slice its columns
        GH_CHECK(slice_uvw(ctx, n, u, v, w, uv_stride, du, dv, dw));
        u = du.as<double>(), v = dv.as<double>(), w = dw.as<double>();
    }
    GH_CHECK_HIP(ctx, hipMemsetAsync(grid, 0, (size_t)N * N * 16, ctx->stream));
    WCache cache;
    GH_CHECK(w_cache_grid_dev(ctx, cache, theta, lam, fn.wstep, qpx, npixFF, npixKern, N, n, u, v, w, vis, grid));
    return st.finish();
}

int gridhip_w_cache_imaging(gridhip_ctx *ctx, int64_t wstep, int64_t qpx, int64_t npixFF, int64_t npixKern,
                            double theta, int64_t lam, int64_t n, const double *u, const double *v, const double *w,
                            int64_t uv_stride, const double *vis, double *grid)
{
    return w_cache_imaging_any(ctx, false, wstep, qpx, npixFF, npixKern, theta, lam, n, u, v, w, uv_stride, vis, grid);
}

int gridhip_w_cache_imaging_dev(gridhip_ctx *ctx, int64_t wstep, int64_t qpx, int64_t npixFF, int64_t npixKern,
                                double theta, int64_t lam, int64_t n, const double *u, const double *v, const double *w,
                                int64_t uv_stride, const double *vis, double *grid)
{
    return w_cache_imaging_any(ctx, true, wstep, qpx, npixFF, npixKern, theta, lam, n, u, v, w, uv_stride, vis, grid);
}

// aw_imaging / aw_imagingOld, src/Gridding.hs:452-506: p = uvw/lam, wbin = findClosest wbins w,
// index = (wbin, a1, a2), then convgrid4 / convgrid3 (same grid).  wvals are the W plane w-values.  The N x N grid is
// overwritten.  The device-resident form is asynchronous: nothing is read back.
static int aw_imaging_any(gridhip_ctx *ctx, bool dev, const AwArgs &a, double *grid)
{
    if (!ctx) return GRIDHIP_EINVAL;
    int64_t N = 0;
    GH_CHECK(aw_check(ctx, a, &N));
    if (!grid) return fail(ctx, GRIDHIP_EINVAL, "bad argument");
    GH_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    Staged st(ctx, dev);
    const AwArgs d = stage_aw(st, a);
    grid = st.out(grid, (size_t)N * N * 16);
    GH_CHECK(st.status());
    GH_CHECK(aw_imaging_to(ctx, N, d, grid));
    return st.finish();
}

int gridhip_aw_imaging(gridhip_ctx *ctx, double theta, int64_t lam, int64_t W, int64_t Q, int64_t S, int64_t A,
                       const double *wkerns, const double *wvals, const double *akerns, int64_t n, const double *u,
                       const double *v, const double *w, int64_t uv_stride, const int64_t *a1, const int64_t *a2,
                       const double *vis, double *grid)
{
    const AwArgs a{theta, lam, W, Q, S, A, wkerns, wvals, akerns, n, u, v, w, uv_stride, a1, a2, vis};
    return aw_imaging_any(ctx, false, a, grid);
}

int gridhip_aw_imaging_dev(gridhip_ctx *ctx, double theta, int64_t lam, int64_t W, int64_t Q, int64_t S, int64_t A,
                           const double *wkerns, const double *wvals, const double *akerns, int64_t n, const double *u,
                           const double *v, const double *w, int64_t uv_stride, const int64_t *a1, const int64_t *a2,
                           const double *vis, double *grid)
{
    const AwArgs a{theta, lam, W, Q, S, A, wkerns, wvals, akerns, n, u, v, w, uv_stride, a1, a2, vis};
    return aw_imaging_any(ctx, true, a, grid);
}

// do_imaging, src/Gridding.hs:509-549, with the ImagingFunction fn (imaging.h).
// dev: every array argument (kv, u, v, w, vis, image, psf) is device-resident; pmax stays a host pointer.
static int do_imaging_any(gridhip_ctx *ctx, bool dev, ImagingFn fn, int64_t n, const double *u, const double *v,
                          const double *w, int64_t uv_stride, const double *vis, double *image, double *psf, double *pmax)
{
    if (!ctx) return GRIDHIP_EINVAL;
    if (n < 0 || uv_stride < 1 || (n > 0 && (!u || !v || !w || !vis))) return fail(ctx, GRIDHIP_EINVAL, "bad argument");
    GH_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    int64_t N = 0;
    GH_CHECK(imaging_fn_check(ctx, fn, &N));
    Staged st(ctx, dev);
    if (fn.kind == 1) fn.kv = st.in(fn.kv, (size_t)fn.Q * fn.Q * fn.gh * fn.gw * 16);  // (no other kind reads it)
    WCache cache;  // w_cache: built by the image pass, reused by the PSF pass
    return do_imaging_impl(ctx, st, N, fn.lam, n, u, v, w, uv_stride, vis, image, psf, pmax,
                           [&](const double *uu, const double *vv, const double *ww, const double *vs, double *g) {
                               if (fn.kind == 0) return simple_grid_dev(ctx, fn.lam, N, n, uu, vv, vs, g);
                               if (fn.kind == 1)
                                   return conv_grid_dev(ctx, fn.lam, N, fn.Q, fn.gh, fn.gw, fn.kv, n, uu, vv, vs, g);
                               return w_cache_grid_dev(ctx, cache, fn.theta, fn.lam, fn.wstep, fn.Q, fn.npixFF, fn.gh, N, n,
                                                       uu, vv, ww, vs, g);
                           });
}

int gridhip_do_imaging(gridhip_ctx *ctx, int kind, int64_t wstep, int64_t Q, int64_t npixFF, int64_t gh, int64_t gw,
                       const double *kv, double theta, int64_t lam, int64_t n, const double *u, const double *v,
                       const double *w, int64_t uv_stride, const double *vis, double *image, double *psf,
                       double *pmax)
{
    return do_imaging_any(ctx, false, {kind, wstep, Q, npixFF, gh, gw, kv, theta, lam}, n, u, v, w, uv_stride, vis, image,
                          psf, pmax);
}

int gridhip_do_imaging_dev(gridhip_ctx *ctx, int kind, int64_t wstep, int64_t Q, int64_t npixFF, int64_t gh, int64_t gw,
                           const double *kv, double theta, int64_t lam, int64_t n, const double *u, const double *v,
                           const double *w, int64_t uv_stride, const double *vis, double *image, double *psf,
                           double *pmax)
{
    return do_imaging_any(ctx, true, {kind, wstep, Q, npixFF, gh, gw, kv, theta, lam}, n, u, v, w, uv_stride, vis, image,
                          psf, pmax);
}

int gridhip_do_imaging_aw(gridhip_ctx *ctx, double theta, int64_t lam, int64_t W, int64_t Q, int64_t S, int64_t A,
                          const double *wkerns, const double *wvals, const double *akerns, int64_t n, const double *u,
                          const double *v, const double *w, int64_t uv_stride, const int64_t *a1, const int64_t *a2,
                          const double *vis, double *image, double *psf, double *pmax)
{
    const AwArgs a{theta, lam, W, Q, S, A, wkerns, wvals, akerns, n, u, v, w, uv_stride, a1, a2, vis};
    return do_imaging_aw_any(ctx, false, a, image, psf, pmax);
}

int gridhip_do_imaging_aw_dev(gridhip_ctx *ctx, double theta, int64_t lam, int64_t W, int64_t Q, int64_t S, int64_t A,
                              const double *wkerns, const double *wvals, const double *akerns, int64_t n, const double *u,
                              const double *v, const double *w, int64_t uv_stride, const int64_t *a1, const int64_t *a2,
                              const double *vis, double *image, double *psf, double *pmax)
{
    const AwArgs a{theta, lam, W, Q, S, A, wkerns, wvals, akerns, n, u, v, w, uv_stride, a1, a2, vis};
    return do_imaging_aw_any(ctx, true, a, image, psf, pmax);
}

int gridhip_aw_gridding(gridhip_ctx *ctx, double theta, int64_t lam, double f, int64_t W, int64_t Q, int64_t S,
                        int64_t A, const double *wkerns, const double *wvals, const double *akerns, int64_t n,
                        const double *u, const double *v, const double *w, int64_t uv_stride, const int64_t *a1,
                        const int64_t *a2, const double *vis, double *image, double *imax)
{
    const AwArgs a{theta, lam, W, Q, S, A, wkerns, wvals, akerns, n, u, v, w, uv_stride, a1, a2, vis};
    return aw_gridding_any(ctx, false, a, f, image, imax);
}

int gridhip_aw_gridding_dev(gridhip_ctx *ctx, double theta, int64_t lam, double f, int64_t W, int64_t Q, int64_t S,
                            int64_t A, const double *wkerns, const double *wvals, const double *akerns, int64_t n,
                            const double *u, const double *v, const double *w, int64_t uv_stride, const int64_t *a1,
                            const int64_t *a2, const double *vis, double *image, double *imax)
{
    const AwArgs a{theta, lam, W, Q, S, A, wkerns, wvals, akerns, n, u, v, w, uv_stride, a1, a2, vis};
    return aw_gridding_any(ctx, true, a, f, image, imax);
}

}  // extern "C"
