// The operations either side of the gridder, on the device: uvw scaling (div3), the w-bin rule and findClosest,
// mirror_uvw, doweight, make_grid_hermitian, the w-kernel generator, the imaging tail and the normalisation, each a
// small kernel with its launcher, and the drop-in entry points that run one of them on host arrays
// (src/Gridding.hs:426-432, 551-605, 610-728, 815-839, 895-907).
//
// Every kernel here is HBM-streaming or tiny; the hot path stays the tile kernel.
#include "common.h"
#include "imaging.h"

namespace gridhip {

// ---------------------------------------------------------------------------------------------
// small kernels

// div3 (src/Gridding.hs:838-839): a true division, not a multiply by the reciprocal
__global__ void scale_kernel(int64_t n, const double *__restrict__ x, int64_t stride, double lam,
                             double *__restrict__ out)
{
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x)
        out[k] = x[k * stride] / lam;
}

// w-bin rule, src/Gridding.hs:426-432: roundedw = wstep * round(w / wstep)
__global__ void wround_kernel(int64_t n, const double *__restrict__ w, int64_t stride, int64_t wstep,
                              int64_t *__restrict__ rw, long long *__restrict__ minmax)
{
    long long mn = 0x7fffffffffffffffLL, mx = -0x7fffffffffffffffLL - 1;
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x) {
        const long long r = (long long)wstep * (long long)round(w[k * stride] / (double)wstep);
        rw[k] = r;
        mn = r < mn ? r : mn;
        mx = r > mx ? r : mx;
    }
    for (int off = 32; off > 0; off >>= 1) {
        long long a = __shfl_xor(mn, off, 64), b = __shfl_xor(mx, off, 64);
        mn = a < mn ? a : mn;
        mx = b > mx ? b : mx;
    }
    // one pair of atomics per work-group (the two 64-bit counters are the same for everybody: one pair per wave was
    // 3 x 10^4 serialised atomics, most of this kernel's 0.39 ms at 10^7 visibilities)
    __shared__ long long smn[16], smx[16];
    const int wave = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    if ((threadIdx.x & 63) == 0) {
        smn[wave] = mn;
        smx[wave] = mx;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < nw; ++i) {
            mn = smn[i] < mn ? smn[i] : mn;
            mx = smx[i] > mx ? smx[i] : mx;
        }
        atomicMin(&minmax[0], mn);
        atomicMax(&minmax[1], mx);
    }
}

__global__ void wbin_finish_kernel(int64_t n, int64_t *__restrict__ rw, int64_t wstep,
                                   const long long *__restrict__ minmax)
{
    const long long mn = minmax[0];
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x)
        rw[k] = (rw[k] - mn) / wstep;  // non-negative: `div` and C division agree
}

// (closest_index: imaging.h)
__global__ void find_closest_kernel(int64_t nws, const double *__restrict__ ws, int64_t n,
                                    const double *__restrict__ w, int64_t stride, int64_t *__restrict__ out)
{
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x)
        out[k] = closest_index(nws, ws, w[k * stride]);
}

// mirror_uvw, src/Gridding.hs:551-562
__global__ void mirror_kernel(int64_t n, double *__restrict__ u, double *__restrict__ v, double *__restrict__ w,
                              double2 *__restrict__ vis)
{
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x) {
        if (v[k] < 0) {
            u[k] = -u[k];
            v[k] = -v[k];
            if (w) w[k] = -w[k];
            if (vis) vis[k].y = -vis[k].y;
        }
    }
}

// doweight, src/Gridding.hs:564-583: frac_coords (N,N) 1 p -> cell histogram -> v / count  (weight_cell: imaging.h)
__global__ void weight_hist_kernel(int64_t N, int64_t n, const double *__restrict__ pu, const double *__restrict__ pv,
                                   unsigned int *__restrict__ cnt)
{
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x) {
        const int64_t c = weight_cell(N, pu[k], pv[k]);
        if (c >= 0) atomicAdd(&cnt[c], 1u);
    }
}

__global__ void weight_apply_kernel(int64_t N, int64_t n, const double *__restrict__ pu, const double *__restrict__ pv,
                                    const unsigned int *__restrict__ cnt, double2 *__restrict__ vis)
{
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x) {
        const int64_t c = weight_cell(N, pu[k], pv[k]);
        if (c < 0) continue;
        const double wgt = (double)cnt[c];
        double2 v = vis[k];
        v.x /= wgt;
        v.y /= wgt;
        vis[k] = v;
    }
}

// make_grid_hermitian, src/Gridding.hs:585-605 (out of place).  `s`: the output is the Hermitian grid rolled by s both
// ways (out[y][x] = H[(y+s) mod N][(x+s) mod N]) - the ishift2D the centred transform starts with, written at once.
__global__ void hermitian_kernel(int64_t N, const double2 *__restrict__ in, double2 *__restrict__ out, int64_t s)
{
    const bool even = (N % 2) == 0;
    const int64_t cells = N * N;
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < cells; c += (int64_t)gridDim.x * blockDim.x) {
        int64_t y = c / N, x = c - y * N;
        y += s;
        x += s;
        y -= y >= N ? N : 0;
        x -= x >= N ? N : 0;
        // the conjugate is ADDED (zipWith (+), :605), and on an even grid's first row and column what is added is 0 :+ 0:
        // an imaginary part of -0.0 becomes +0.0 there (g.y - 0.0 would keep -0.0)
        double2 a = make_double2(0.0, 0.0);
        if (!even || (x != 0 && y != 0)) {
            a = even ? in[(N - y) * N + (N - x)] : in[(N - 1 - y) * N + (N - 1 - x)];
            a.y = -a.y;
        }
        const double2 g = in[y * N + x];
        out[c] = make_double2(g.x + a.x, g.y + a.y);
    }
}

// out[y][x] = in[(y+s) mod N][(x+s) mod N] * scale   (shift2D: s = ceil(N/2), ishift2D: s = floor(N/2))
__global__ void roll_kernel(int64_t N, const double2 *__restrict__ in, double2 *__restrict__ out, int64_t s,
                            double scale)
{
    const int64_t cells = N * N;
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < cells; c += (int64_t)gridDim.x * blockDim.x) {
        const int64_t y = c / N, x = c - y * N;
        int64_t sy = y + s, sx = x + s;
        sy -= sy >= N ? N : 0;
        sx -= sx >= N ? N : 0;
        const double2 v = in[sy * N + sx];
        out[c] = make_double2(v.x * scale, v.y * scale);
    }
}

// N > 0: `in` is a transform's raw N x N output and the cell read for c = (y, x) is in[(y+s) mod N][(x+s) mod N] * scale -
// the shift2D and the 1 / N^2 the centred inverse transform ends with, applied while the real part is taken instead
// of in a pass of their own (the same multiplication: bit-identical).
// DIV (an imager's cycle: the PSF's maximum is known beforehand): the real part is stored divided by the maximum that
// divbits holds in divide_kernel's form - that kernel's division, without its pass - and no maximum is taken.
template <bool DIV>
__global__ void real_max_kernel(int64_t cells, const double2 *__restrict__ in, double *__restrict__ real_out,
                                unsigned long long *__restrict__ maxbits, int64_t N, int64_t s, double scale,
                                const unsigned long long *__restrict__ divbits)
{
    double m = -INFINITY;
    double dm = 1.0;
    if (DIV) dm = ordered_value(*divbits);
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < cells; c += (int64_t)gridDim.x * blockDim.x) {
        double r;
        if (N > 0) {
            int64_t y = c / N, x = c - y * N;
            y += s;
            x += s;
            y -= y >= N ? N : 0;
            x -= x >= N ? N : 0;
            r = in[y * N + x].x * scale;
        } else
            r = in[c].x;
        if (DIV) {
            real_out[c] = r / dm;
            continue;
        }
        if (real_out) real_out[c] = r;
        m = r > m ? r : m;
    }
    if (DIV) return;
    for (int off = 32; off > 0; off >>= 1) {
        const double o = __shfl_xor(m, off, 64);
        m = o > m ? o : m;
    }
    // one atomic per work-group (one per wave was 1.6 x 10^4 serialised 64-bit atomics on one address: most of this
    // kernel's 0.11 ms at 2400^2 cells)
    __shared__ double sm[16];
    const int wave = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    if ((threadIdx.x & 63) == 0) sm[wave] = m;
    __syncthreads();
    if (threadIdx.x == 0 && maxbits) {
        for (int i = 1; i < nw; ++i) m = sm[i] > m ? sm[i] : m;
        atomicMax(maxbits, ordered_bits(m));
    }
}

__global__ void divide_kernel(int64_t cells, double *__restrict__ x, const unsigned long long *__restrict__ maxbits)
{
    const double m = ordered_value(*maxbits);
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < cells; c += (int64_t)gridDim.x * blockDim.x)
        x[c] /= m;
}

// w_kernel far field, padded (src/Gridding.hs:610-667, pad_mid :682-691 via padder :863-877).
// padder reads `array ! index2 oldx oldy`: the far field is transposed while it is padded.
// `s`: the output is the padded far field rolled by s both ways (out[y][x] = field[(y+s) mod na][(x+s) mod na]) - the
// ishift2D the centred transform starts with, written at once instead of by a pass of its own.
__global__ void wkern_farfield_kernel(int64_t n, int64_t na, double theta, double w, double2 *__restrict__ out, int64_t s)
{
    const int64_t p0 = na / 2 - n / 2;
    const double step = 1.0 / (double)n;
    const double start = (double)(-(n / 2)) * step;
    const int64_t cells = na * na;
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < cells; c += (int64_t)gridDim.x * blockDim.x) {
        int64_t y = c / na, x = c - y * na;
        y += s;
        x += s;
        y -= y >= na ? na : 0;
        x -= x >= na ? na : 0;
        int64_t oldx = x - p0, oldy = y - p0;
        double2 v = make_double2(0.0, 0.0);
        if (n == na) {  // pad_mid returns ff untouched
            oldx = y;
            oldy = x;
        }
        if (oldx >= 0 && oldx < n && oldy >= 0 && oldy < n) {
            // ff[row = oldx][col = oldy]: l = base[col] * theta, m = base[row] * theta
#pragma clang fp contract(off)
            const double l = (start + (double)oldy * step) * theta;
            const double m = (start + (double)oldx * step) * theta;
            const double r2 = l * l + m * m;
            const double ph = 1.0 - sqrt(1.0 - r2);
            const double arg = 2.0 * M_PI * w * ph;
            double sn, cs;
            sincos(arg, &sn, &cs);
            v = make_double2(cs, sn);
        }
        out[c] = v;
    }
}

// extract_oversampled, src/Gridding.hs:709-728: K[yf,xf,y,x] = af[c - yf + Q*y, c - xf + Q*x] * Q^2
// `s`, `scale`: af is the transform's raw output; the cell the reference reads is af[(row+s) mod na][(col+s) mod na] *
// scale - the shift2D and the 1 / na^2 the centred inverse transform ends with, applied to the Q^2 S^2 cells that are
// used instead of to all na^2 (same two multiplications in the same order: bit-identical).
__global__ void wkern_extract_kernel(int64_t na, int64_t Q, int64_t S, const double2 *__restrict__ af,
                                     double2 *__restrict__ out, int conj, int64_t s, double scale)
{
    const int64_t c0 = na / 2 - Q * (S / 2);
    const double q2 = (double)(Q * Q);
    const int64_t total = Q * Q * S * S;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        int64_t r = t;
        const int64_t x = r % S;
        r /= S;
        const int64_t y = r % S;
        r /= S;
        const int64_t xf = r % Q, yf = r / Q;
        int64_t row = c0 - yf + Q * y + s, col = c0 - xf + Q * x + s;
        row -= row >= na ? na : 0;
        col -= col >= na ? na : 0;
        double2 v = af[row * na + col];
        v = make_double2(v.x * scale, v.y * scale);
        out[t] = make_double2(v.x * q2, conj ? -(v.y * q2) : v.y * q2);
    }
}

int launch_scale(gridhip_ctx *ctx, int64_t n, const double *x, int64_t stride, double lam, double *out)
{
    if (n > 0) hipLaunchKernelGGL(scale_kernel, grid_for(ctx, n), dim3(256), 0, ctx->stream, n, x, stride, lam, out);
    GH_CHECK_HIP(ctx, hipGetLastError());
    return GRIDHIP_OK;
}

int scaled_uv(gridhip_ctx *ctx, int64_t n, const double *u, const double *v, int64_t stride, double lam, DevBuf &pu,
              DevBuf &pv)
{
    GH_CHECK(pu.alloc(ctx, (size_t)n * 8));
    GH_CHECK(pv.alloc(ctx, (size_t)n * 8));
    GH_CHECK(launch_scale(ctx, n, u, stride, lam, pu.as<double>()));
    return launch_scale(ctx, n, v, stride, lam, pv.as<double>());
}

// (a division by 1 is exact: scale_kernel serves as the strided copy)
int slice_uvw(gridhip_ctx *ctx, int64_t n, const double *u, const double *v, const double *w, int64_t stride, DevBuf &du,
              DevBuf &dv, DevBuf &dw)
{
    GH_CHECK(scaled_uv(ctx, n, u, v, stride, 1.0, du, dv));
    GH_CHECK(dw.alloc(ctx, (size_t)n * 8));
    return w ? launch_scale(ctx, n, w, stride, 1.0, dw.as<double>()) : GRIDHIP_OK;
}

int launch_mirror(gridhip_ctx *ctx, int64_t n, double *u, double *v, double *w, double2 *vis)
{
    if (n > 0) hipLaunchKernelGGL(mirror_kernel, grid_for(ctx, n), dim3(256), 0, ctx->stream, n, u, v, w, vis);
    GH_CHECK_HIP(ctx, hipGetLastError());
    return GRIDHIP_OK;
}

int launch_doweight(gridhip_ctx *ctx, int64_t N, int64_t n, const double *pu, const double *pv, unsigned int *cnt,
                    double2 *vis)
{
    if (n > 0) {
        hipLaunchKernelGGL(weight_hist_kernel, grid_for(ctx, n), dim3(256), 0, ctx->stream, N, n, pu, pv, cnt);
        hipLaunchKernelGGL(weight_apply_kernel, grid_for(ctx, n), dim3(256), 0, ctx->stream, N, n, pu, pv, cnt, vis);
    }
    GH_CHECK_HIP(ctx, hipGetLastError());
    return GRIDHIP_OK;
}

int launch_divide(gridhip_ctx *ctx, int64_t cells, double *x, const unsigned long long *maxbits)
{
    hipLaunchKernelGGL(divide_kernel, grid_for(ctx, cells), dim3(256), 0, ctx->stream, cells, x, maxbits);
    GH_CHECK_HIP(ctx, hipGetLastError());
    return GRIDHIP_OK;
}

int launch_roll(gridhip_ctx *ctx, int64_t N, const double2 *in, double2 *out, int64_t s, double scale)
{
    hipLaunchKernelGGL(roll_kernel, grid_for(ctx, N * N), dim3(256), 0, ctx->stream, N, in, out, s, scale);
    GH_CHECK_HIP(ctx, hipGetLastError());
    return GRIDHIP_OK;
}

// one plane of the w-kernel table: out[Q][Q][S][S] (conjugated when the caller is w_cache_imaging, :441)
int dev_w_kernel(gridhip_ctx *ctx, double theta, double w, int64_t npixFF, int64_t S, int64_t Q, double2 *out,
                 bool conj, double2 *pad)
{
    const int64_t na = npixFF * Q;
    // centred inverse transform = shift2D . ifft2D . ishift2D (dev_fft2c); its two rolls are folded into the far-field
    // kernel's stores and the extraction's loads: three passes over na^2 cells fewer per plane
    void *plan = nullptr;
    GH_CHECK(fft_plan_for(ctx, na, &plan));
    hipLaunchKernelGGL(wkern_farfield_kernel, grid_for(ctx, na * na), dim3(256), 0, ctx->stream, npixFF, na, theta, w,
                       pad, na / 2);
    GH_CHECK(fft_exec(ctx, plan, pad, true));
    hipLaunchKernelGGL(wkern_extract_kernel, grid_for(ctx, Q * Q * S * S), dim3(256), 0, ctx->stream, na, Q, S, pad,
                       out, conj ? 1 : 0, (na + 1) / 2, 1.0 / ((double)na * (double)na));
    GH_CHECK_HIP(ctx, hipGetLastError());
    return GRIDHIP_OK;
}

// w-bins on the device; returns min and plane count to the host (the reference does the same
// round-trip with a nested CPU.run, :430)
int dev_wbins(gridhip_ctx *ctx, int64_t n, const double *w, int64_t stride, int64_t wstep, int64_t *wbin,
                     int64_t *wmin, int64_t *nplanes)
{
    DevBuf mm;
    const long long init[2] = {0x7fffffffffffffffLL, -0x7fffffffffffffffLL - 1};
    GH_CHECK(mm.upload(ctx, init, 16));
    if (n > 0) {
        hipLaunchKernelGGL(wround_kernel, dim3(grid_for(ctx, n).x > (unsigned)ctx->num_cu * 4 ? (unsigned)ctx->num_cu * 4 : grid_for(ctx, n).x), dim3(256), 0, ctx->stream, n, w, stride, wstep, wbin,
                           mm.as<long long>());
        hipLaunchKernelGGL(wbin_finish_kernel, grid_for(ctx, n), dim3(256), 0, ctx->stream, n, wbin, wstep,
                           mm.as<long long>());
    }
    long long res[2];
    GH_CHECK(d2h(ctx, res, mm.p, 16));
    GH_CHECK(sync(ctx));
    GH_CHECK_HIP(ctx, hipGetLastError());
    *wmin = n > 0 ? res[0] : 0;
    *nplanes = n > 0 ? (res[1] - res[0]) / wstep + 1 : 0;
    return GRIDHIP_OK;
}

// out = real(ifft(make_grid_hermitian(g))) (N x N doubles), its maximum into *maxbits (ordered bits) when given: the
// imaging tail (src/Gridding.hs:539,542).  The centred inverse transform (shift2D . ifft2D . ishift2D, dev_fft2c) has its
// two rolls folded into the Hermitian fill's stores and the real part's loads: four passes over the N^2 grid fewer per
// call.  h: N x N complex scratch.  divbits (an imager's cycle; maxbits is then null): out is stored divided by the
// maximum kept there.  plan: the caller's own transform (fft_plan_own) instead of the context's cached one.
int image_tail(gridhip_ctx *ctx, int64_t N, const double2 *g, double2 *h, double *out, unsigned long long *maxbits,
               const unsigned long long *divbits, void *plan)
{
    static const unsigned long long neg_inf_bits = ordered_bits(-INFINITY);  // (static: the source of an async copy)
    const size_t cells = (size_t)N * N;
    if (plan)
        GH_CHECK(fft_plan_bind(ctx, plan));
    else
        GH_CHECK(fft_plan_for(ctx, N, &plan));
    hipLaunchKernelGGL(hermitian_kernel, grid_for(ctx, cells), dim3(256), 0, ctx->stream, N, g, h, N / 2);
    GH_CHECK(fft_exec(ctx, plan, h, true));
    if (maxbits) GH_CHECK(h2d(ctx, maxbits, &neg_inf_bits, 8));
    if (divbits)
        hipLaunchKernelGGL(real_max_kernel<true>, dim3((unsigned)ctx->num_cu * 4), dim3(256), 0, ctx->stream, (int64_t)cells,
                           h, out, (unsigned long long *)nullptr, N, (N + 1) / 2, 1.0 / ((double)N * (double)N), divbits);
    else
        hipLaunchKernelGGL(real_max_kernel<false>, dim3((unsigned)ctx->num_cu * 4), dim3(256), 0, ctx->stream, (int64_t)cells,
                           h, out, maxbits, N, (N + 1) / 2, 1.0 / ((double)N * (double)N),
                           (const unsigned long long *)nullptr);
    GH_CHECK_HIP(ctx, hipGetLastError());
    return GRIDHIP_OK;
}

// normalise image and PSF by the PSF's maximum (src/Gridding.hs:544-548): maxbits holds it (image_tail), *pmax gets it
int normalise(gridhip_ctx *ctx, size_t cells, double *image, double *psf, const unsigned long long *maxbits, double *pmax)
{
    GH_CHECK(launch_divide(ctx, (int64_t)cells, image, maxbits));
    GH_CHECK(launch_divide(ctx, (int64_t)cells, psf, maxbits));
    unsigned long long mb = 0;
    GH_CHECK(d2h(ctx, &mb, maxbits, 8));
    GH_CHECK(sync(ctx));
    if (pmax) *pmax = ordered_value(mb);
    return GRIDHIP_OK;
}

// [nplanes][Q][Q][S][S] w-kernels of the planes w = i * wstep + wmin (:434-448), conjugated or not.  Asynchronous.
int build_w_planes(gridhip_ctx *ctx, double theta, int64_t wstep, int64_t wmin, int64_t nplanes, int64_t npixFF, int64_t S,
                   int64_t Q, double2 *table, bool conj)
{
    const int64_t na = npixFF * Q;
    DevBuf pad;
    GH_CHECK(pad.alloc(ctx, (size_t)na * na * 16));
    for (int64_t i = 0; i < nplanes; ++i)
        GH_CHECK(dev_w_kernel(ctx, theta, (double)(i * wstep + wmin), npixFF, S, Q, table + i * Q * Q * S * S, conj,
                              pad.as<double2>()));
    return GRIDHIP_OK;
}

}  // namespace gridhip

using namespace gridhip;

extern "C" {

// Prelude `round` on the host (N = round (theta * lam), src/Gridding.hs:87,118,416): half to even
int64_t gridhip_image_size(double theta, int64_t lam) { return (int64_t)nearbyint(theta * (double)lam); }

int gridhip_wbins(gridhip_ctx *ctx, int64_t n, const double *w, int64_t wstep, int64_t *wbin, int64_t *wmin,
                  int64_t *nplanes)
{
    if (!ctx) return GRIDHIP_EINVAL;
    if (n < 0 || wstep <= 0 || (n > 0 && (!w || !wbin)) || !wmin || !nplanes)
        return fail(ctx, GRIDHIP_EINVAL, "bad argument");
    GH_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    DevBuf dw, db;
    GH_CHECK(dw.upload(ctx, w, n * 8));
    GH_CHECK(db.alloc(ctx, n * 8));
    GH_CHECK(dev_wbins(ctx, n, dw.as<double>(), 1, wstep, db.as<int64_t>(), wmin, nplanes));
    GH_CHECK(d2h(ctx, wbin, db.p, n * 8));
    return sync(ctx);
}

int gridhip_find_closest(gridhip_ctx *ctx, int64_t nws, const double *ws, int64_t n, const double *w, int64_t *out)
{
    if (!ctx) return GRIDHIP_EINVAL;
    if (nws <= 0 || n < 0 || !ws || (n > 0 && (!w || !out))) return fail(ctx, GRIDHIP_EINVAL, "bad argument");
    GH_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    DevBuf dws, dw, dout;
    GH_CHECK(dws.upload(ctx, ws, nws * 8));
    GH_CHECK(dw.upload(ctx, w, n * 8));
    GH_CHECK(dout.alloc(ctx, n * 8));
    if (n > 0)
        hipLaunchKernelGGL(find_closest_kernel, grid_for(ctx, n), dim3(256), 0, ctx->stream, nws, dws.as<double>(), n,
                           dw.as<double>(), (int64_t)1, dout.as<int64_t>());
    GH_CHECK_HIP(ctx, hipGetLastError());
    GH_CHECK(d2h(ctx, out, dout.p, n * 8));
    return sync(ctx);
}

int gridhip_mirror_uvw(gridhip_ctx *ctx, int64_t n, double *u, double *v, double *w, double *vis)
{
    if (!ctx) return GRIDHIP_EINVAL;
    if (n < 0 || (n > 0 && (!u || !v))) return fail(ctx, GRIDHIP_EINVAL, "bad argument");
    GH_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    DevBuf du, dv, dw, dvis;
    GH_CHECK(du.upload(ctx, u, n * 8));
    GH_CHECK(dv.upload(ctx, v, n * 8));
    GH_CHECK(dw.upload(ctx, w, w ? n * 8 : 0));
    GH_CHECK(dvis.upload(ctx, vis, vis ? n * 16 : 0));
    GH_CHECK(launch_mirror(ctx, n, du.as<double>(), dv.as<double>(), w ? dw.as<double>() : nullptr,
                           vis ? dvis.as<double2>() : nullptr));
    GH_CHECK(d2h(ctx, u, du.p, n * 8));
    GH_CHECK(d2h(ctx, v, dv.p, n * 8));
    if (w) GH_CHECK(d2h(ctx, w, dw.p, n * 8));
    if (vis) GH_CHECK(d2h(ctx, vis, dvis.p, n * 16));
    return sync(ctx);
}

int gridhip_doweight(gridhip_ctx *ctx, double theta, int64_t lam, int64_t n, const double *u, const double *v,
                     double *vis)
{
    if (!ctx) return GRIDHIP_EINVAL;
    const int64_t N = gridhip_image_size(theta, lam);
    if (N <= 0 || n < 0 || (n > 0 && (!u || !v || !vis))) return fail(ctx, GRIDHIP_EINVAL, "bad argument");
    GH_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    DevBuf du, dv, dpu, dpv, dvis, cnt;
    GH_CHECK(du.upload(ctx, u, n * 8));
    GH_CHECK(dv.upload(ctx, v, n * 8));
    GH_CHECK(dvis.upload(ctx, vis, n * 16));
    GH_CHECK(cnt.alloc(ctx, (size_t)N * N * 4));
    GH_CHECK_HIP(ctx, hipMemsetAsync(cnt.p, 0, (size_t)N * N * 4, ctx->stream));
    GH_CHECK(scaled_uv(ctx, n, du.as<double>(), dv.as<double>(), 1, (double)lam, dpu, dpv));
    GH_CHECK(launch_doweight(ctx, N, n, dpu.as<double>(), dpv.as<double>(), cnt.as<unsigned int>(), dvis.as<double2>()));
    GH_CHECK(d2h(ctx, vis, dvis.p, n * 16));
    return sync(ctx);
}

int gridhip_make_grid_hermitian(gridhip_ctx *ctx, int64_t N, double *grid)
{
    if (!ctx) return GRIDHIP_EINVAL;
    if (N <= 0 || !grid) return fail(ctx, GRIDHIP_EINVAL, "bad argument");
    GH_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    const size_t cells = (size_t)N * N;
    DevBuf a, b;
    GH_CHECK(a.upload(ctx, grid, cells * 16));
    GH_CHECK(b.alloc(ctx, cells * 16));
    hipLaunchKernelGGL(hermitian_kernel, grid_for(ctx, cells), dim3(256), 0, ctx->stream, N, a.as<double2>(),
                       b.as<double2>(), (int64_t)0);
    GH_CHECK_HIP(ctx, hipGetLastError());
    GH_CHECK(d2h(ctx, grid, b.p, cells * 16));
    return sync(ctx);
}

int gridhip_fft2_centered(gridhip_ctx *ctx, int64_t N, const double *in, double *out, int inverse)
{
    if (!ctx) return GRIDHIP_EINVAL;
    if (N <= 0 || !in || !out) return fail(ctx, GRIDHIP_EINVAL, "bad argument");
    GH_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    const size_t cells = (size_t)N * N;
    DevBuf a, b, t;
    GH_CHECK(a.upload(ctx, in, cells * 16));
    GH_CHECK(b.alloc(ctx, cells * 16));
    GH_CHECK(t.alloc(ctx, cells * 16));
    GH_CHECK(dev_fft2c(ctx, N, a.as<double2>(), b.as<double2>(), t.as<double2>(), inverse != 0));
    GH_CHECK(d2h(ctx, out, b.p, cells * 16));
    return sync(ctx);
}

int gridhip_w_kernel(gridhip_ctx *ctx, double theta, double w, int64_t npixFF, int64_t npixKern, int64_t qpx,
                     double *out)
{
    if (!ctx) return GRIDHIP_EINVAL;
    if (!out) return fail(ctx, GRIDHIP_EINVAL, "bad argument");
    if (!w_kernel_shape_ok(npixFF, npixKern, qpx))
        return fail(ctx, GRIDHIP_EINVAL, "w-kernel shape npixFF %lld, npixKern %lld, qpx %lld: not positive, npixKern > npixFF, "
                    "or extracting outside the far field", (long long)npixFF, (long long)npixKern, (long long)qpx);
    GH_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    const int64_t na = npixFF * qpx;
    const size_t kel = (size_t)qpx * qpx * npixKern * npixKern;
    DevBuf pad, k;
    GH_CHECK(pad.alloc(ctx, na * na * 16));
    GH_CHECK(k.alloc(ctx, kel * 16));
    GH_CHECK(dev_w_kernel(ctx, theta, w, npixFF, npixKern, qpx, k.as<double2>(), false, pad.as<double2>()));
    GH_CHECK(d2h(ctx, out, k.p, kel * 16));
    return sync(ctx);
}

}  // extern "C"
