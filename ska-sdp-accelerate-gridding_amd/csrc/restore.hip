// The restoring beam and the restore step (include/gridhip.h, "restoring beam and restore"): what turns clean's model of
// delta components and its residual into a map, without leaving the device.
//
//     fit_beam_kernel   one work-group: the weighted log-quadratic fit of an elliptical Gaussian to the PSF's main lobe.
//                       Each thread owns whole rows of the window and sums its row's nine normal-equation terms (and
//                       the cell count) in dx order; thread 0 adds the rows in dy order, solves the 3 x 3 system by
//                       Cramer's rule and writes the 8 doubles.  No atomics, contraction off: a numpy restatement
//                       (tests/restore_ref.py) differs by its log alone.
//     restore_kernel    restored = residual + model (*) beam, an LDS-tiled direct convolution in fp64.  A work-group of
//                       256 threads makes a tile of RS_TH rows x RS_TW columns; thread (lx, ly) makes the 8 adjacent
//                       cells 8 lx .. 8 lx + 7 of row ly.  The model tile and its halo of `support` cells are staged in
//                       LDS with coalesced row loads (zeros outside the image), and while staging the work-group finds
//                       out whether the window holds any non-zero cell: if not, the tile is residual + 0.0 and neither
//                       the weights nor the taps are evaluated (a CLEAN model is almost entirely zero).  Otherwise the
//                       (2 support + 1)^2 weights are evaluated once into LDS and every thread runs the taps dy
//                       ascending, dx ascending, one fused multiply-add each, from +0.0.
// Why 8 adjacent cells per thread: along dx the model values a thread needs slide by one cell per tap, so a chunk of 8
// taps for 8 cells reads 8 new model values and 8 weights from LDS for 64 multiply-adds - 0.25 LDS reads per
// multiply-add, half of what the LDS delivers beside the fp64 rate (one 64-lane ds_read_b64 per 2 clocks per CU against
// one 64-lane multiply-add per clock per CU).  The weight reads are broadcasts.
// LDS layout: cell u of a staged row lies at u + u / 8, so that lanes 8 cells apart are 9 doubles apart, and the row
// stride is 8 modulo 32 doubles: the 8 x 4 lanes of one 32-lane group of a ds_read_b64 then fall on the 32 distinct
// bank pairs (9 lx mod 32 = {0, 9, 18, 27, 4, 13, 22, 31}, shifted by 0, 8, 16, 24 for the four rows: disjoint), so the
// model reads are conflict-free.  At support 32 the staged window is 96 rows x 168 doubles = 129 024 B and the weights
// 33 800 B: 162 824 B of the 163 840 B a work-group may take.  Smaller supports take less and several work-groups share
// a CU (support 8: 42 KB, three of them).
#include "common.h"
#include "imaging.h"

namespace gridhip {

namespace {

// (the tile RS_TH x RS_TW and the staged layout - staged_pos, staged_stride, restore_lds_bytes - are in imaging.h:
// msclean.hip's set-up convolution shares them)
constexpr int FIT_T = 128;                              // rows of the window one pass of the fit takes

// ---- the fit -----------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(FIT_T)
    fit_beam_kernel(int64_t N, const double *__restrict__ psf, int64_t window, double cut, double *__restrict__ beam)
{
#pragma clang fp contract(off)
    __shared__ double part[FIT_T][10];
    const int t = threadIdx.x;
    const int64_t c = N / 2;
    int64_t R = window < c ? window : c;
    if (N - 1 - c < R) R = N - 1 - c;
    const double pc = psf[c * N + c];
    double tot[10];
    for (int i = 0; i < 10; ++i) tot[i] = 0.0;
    for (int64_t row0 = -R; row0 <= R; row0 += FIT_T) {
        const int64_t dy = row0 + t;
        double s[10];
        for (int i = 0; i < 10; ++i) s[i] = 0.0;
        if (dy <= R) {
            const double *row = psf + (c + dy) * N + c;
            const int64_t ady = dy < 0 ? -dy : dy;
            for (int64_t dx = -R; dx <= R; ++dx) {
                if (dy == 0 && dx == 0) continue;
                const double p = row[dx] / pc;
                const int64_t adx = dx < 0 ? -dx : dx;
                const bool near = (ady > adx ? ady : adx) == 1;
                if (!(p <= 1.0 && (p >= cut || (near && p > 0.0)))) continue;  // (a NaN fails p <= 1)
                const double w = p * p, l = log(p);
                const double a = (double)(dx * dx), b = (double)(2 * dx * dy), cc = (double)(dy * dy);
                const double wa = w * a, wb = w * b, wc = w * cc;
                s[0] += wa * a, s[1] += wa * b, s[2] += wa * cc, s[3] += wb * b, s[4] += wb * cc, s[5] += wc * cc;
                s[6] += wa * l, s[7] += wb * l, s[8] += wc * l;
                s[9] += 1.0;
            }
        }
        for (int i = 0; i < 10; ++i) part[t][i] = s[i];
        __syncthreads();
        if (t == 0) {
            const int64_t rows = R - row0 + 1 < FIT_T ? R - row0 + 1 : FIT_T;
            for (int64_t r = 0; r < rows; ++r)
                for (int i = 0; i < 10; ++i) tot[i] += part[r][i];
        }
        __syncthreads();
    }
    if (t != 0) return;
    // M x = -g for x = (A, B, C); M symmetric: m00 m01 m02 / m11 m12 / m22
    const double m00 = tot[0], m01 = tot[1], m02 = tot[2], m11 = tot[3], m12 = tot[4], m22 = tot[5];
    const double r0 = -tot[6], r1 = -tot[7], r2 = -tot[8];
    const double c00 = m11 * m22 - m12 * m12, c01 = m01 * m22 - m12 * m02, c02 = m01 * m12 - m11 * m02;
    const double det = m00 * c00 - m01 * c01 + m02 * c02;
    const double A = (r0 * c00 - m01 * (r1 * m22 - m12 * r2) + m02 * (r1 * m12 - m11 * r2)) / det;
    const double B = (m00 * (r1 * m22 - m12 * r2) - r0 * c01 + m02 * (m01 * r2 - r1 * m02)) / det;
    const double C = (m00 * (m11 * r2 - r1 * m12) - m01 * (m01 * r2 - r1 * m02) + r0 * c02) / det;
    const bool ok = tot[9] >= 3.0 && det > 0.0 && pc > 0.0 && pc < __builtin_inf() && A > 0.0 && C > 0.0 &&
                    A * C - B * B > 0.0 && A < __builtin_inf() && C < __builtin_inf();
    if (!ok) {
        const double nan = __builtin_nan("");
        for (int i = 0; i < 6; ++i) beam[i] = nan;
        beam[6] = tot[9];
        beam[7] = 0.0;
        return;
    }
    const double h = 0.5 * (A + C), d = 0.5 * (A - C), q = sqrt(d * d + B * B);
    const double ln2 = 0.693147180559945309417;
    double pa = (A == C && B == 0.0) ? 0.0 : 0.5 * atan2(0.0 - 2.0 * B, C - A);
    if (pa <= -1.57079632679489661923) pa += 3.14159265358979323846;
    beam[0] = A, beam[1] = B, beam[2] = C;
    beam[3] = 2.0 * sqrt(ln2 / (h - q));
    beam[4] = 2.0 * sqrt(ln2 / (h + q));
    beam[5] = pa;
    beam[6] = tot[9];
    beam[7] = 1.0;
}

// ---- the restore -------------------------------------------------------------------------------------------------------
// (beam_usable - ok set, A, B, C finite and positive definite - is in imaging.h: sources.hip shares it)
// grid (ceil(N / RS_TW), ceil(N / RS_TH)); dynamic LDS: restore_lds_bytes(s); stride = staged_stride(s).
// restored may be residual itself: a cell is read and written by the same thread.
__global__ void __launch_bounds__(256)
    restore_kernel(int64_t N, const double *__restrict__ model, const double *residual, const double *__restrict__ beam,
                   int s, int stride, double *restored)
{
    extern __shared__ __align__(16) double lds[];
    const int t = threadIdx.x, lx = t % RS_LX, ly = t / RS_LX;
    const int64_t x0 = (int64_t)blockIdx.x * RS_TW, y0 = (int64_t)blockIdx.y * RS_TH;
    const int64_t y = y0 + ly, xf = x0 + 8 * lx;  // this thread's row and first cell
    const double A = beam[0], B = beam[1], C = beam[2];
    if (!beam_usable(A, B, C, beam[7])) {  // (uniform over the launch)
        if (y < N)
            for (int j = 0; j < 8; ++j)
                if (xf + j < N) restored[y * N + xf + j] = __builtin_nan("");
        return;
    }
    const int rows = RS_TH + 2 * s, cols = RS_TW + 2 * s, K = 2 * s + 1;
    double *wt = lds + (size_t)rows * stride;
    int any = 0;
    for (int i = t; i < rows * cols; i += 256) {
        const int r = i / cols, u = i - r * cols;
        const int64_t gy = y0 - s + r, gx = x0 - s + u;
        double v = 0.0;
        if (gy >= 0 && gy < N && gx >= 0 && gx < N) v = model[gy * N + gx];
        any |= v != 0.0;  // (true for a NaN)
        lds[r * stride + staged_pos(u)] = v;
    }
    any = __syncthreads_or(any);
    double acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.0;
    if (any) {
        {
#pragma clang fp contract(off)
            for (int i = t; i < K * K; i += 256) {
                const int iy = i / K;
                const double dy = (double)(iy - s), dx = (double)(i - iy * K - s);
                wt[i] = exp(-(A * dx * dx + 2.0 * B * dx * dy + C * dy * dy));
            }
        }
        __syncthreads();
        for (int dy = -s; dy <= s; ++dy) {
            const double *mrow = lds + (ly + s - dy) * stride + 9 * lx;  // cell 8 lx + k of the row: mrow[k + k / 8]
            const double *wrow = wt + (dy + s) * K + s;                  // wrow[dx]
            // tap dx of cell j reads cell k = s - dx + j.  A chunk of 8 taps from dx0: W[e + 7] = cell kb + e, kb = s - dx0,
            // e = j - (dx - dx0) in -7 .. 7; the next chunk keeps W[0 .. 6] as its W[8 .. 14].  The taps left over after
            // the whole chunks (K is odd: 1, 3, 5 or 7 of them) read their cells one by one.
            double W[15];
            int kb = 2 * s, dx0 = -s;
#pragma unroll
            for (int e = 1; e < 8; ++e) W[e + 7] = mrow[staged_pos(kb + e)];
            for (int c = 0; c < K / 8; ++c, dx0 += 8, kb -= 8) {
#pragma unroll
                for (int e = -7; e <= 0; ++e) W[e + 7] = mrow[staged_pos(kb + e)];
#pragma unroll
                for (int d = 0; d < 8; ++d) {
                    const double w = wrow[dx0 + d];
#pragma unroll
                    for (int j = 0; j < 8; ++j) acc[j] = fma(W[j - d + 7], w, acc[j]);
                }
#pragma unroll
                for (int e = 0; e < 7; ++e) W[e + 8] = W[e];
            }
            for (; dx0 <= s; ++dx0, --kb) {
                const double w = wrow[dx0];
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[j] = fma(mrow[staged_pos(kb + j)], w, acc[j]);
            }
        }
    }
    if (y < N)
        for (int j = 0; j < 8; ++j)
            if (xf + j < N) restored[y * N + xf + j] = residual[y * N + xf + j] + acc[j];
}

}  // namespace

int fit_beam_check(gridhip_ctx *ctx, int64_t N, const double *psf, int64_t window, double cut, const double *beam)
{
    if (N < 1 || window < 1 || !(cut > 0.0 && cut < 1.0) || !psf || !beam)
        return fail(ctx, GRIDHIP_EINVAL, "fit_beam: bad argument");
    if (N > CLEAN_MAX_N) return fail(ctx, GRIDHIP_EUNSUPPORTED, "fit_beam: N above %lld", (long long)CLEAN_MAX_N);
    if (overlap(psf, (size_t)N * N * 8, beam, 64)) return fail(ctx, GRIDHIP_EINVAL, "fit_beam: beam must not overlap psf");
    return GRIDHIP_OK;
}

int fit_beam_run(gridhip_ctx *ctx, int64_t N, const double *psf, int64_t window, double cut, double *beam)
{
    hipLaunchKernelGGL(fit_beam_kernel, dim3(1), dim3(FIT_T), 0, ctx->stream, N, psf, window, cut, beam);
    GH_CHECK_HIP(ctx, hipGetLastError());
    return GRIDHIP_OK;
}

int restore_check(gridhip_ctx *ctx, int64_t N, const double *model, const double *residual, const double *beam,
                  int64_t support, const double *restored)
{
    if (N < 1 || support < 1 || !model || !residual || !beam || !restored)
        return fail(ctx, GRIDHIP_EINVAL, "restore: bad argument");
    if (support > 32) return fail(ctx, GRIDHIP_EUNSUPPORTED, "restore: support above 32");
    if (N > CLEAN_MAX_N) return fail(ctx, GRIDHIP_EUNSUPPORTED, "restore: N above %lld", (long long)CLEAN_MAX_N);
    const size_t bytes = (size_t)N * N * 8;
    if (overlap(restored, bytes, model, bytes) || (restored != residual && overlap(restored, bytes, residual, bytes)) ||
        overlap(restored, bytes, beam, 64))
        return fail(ctx, GRIDHIP_EINVAL, "restore: restored may be residual itself, and overlap nothing else");
    return GRIDHIP_OK;
}

int restore_run(gridhip_ctx *ctx, int64_t N, const double *model, const double *residual, const double *beam,
                int64_t support, double *restored)
{
    const int s = (int)support;
    if (!ctx->img->restore_lds_raised) {  // (a work-group may take more than 64 KB only once the function is told so)
        GH_CHECK_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(restore_kernel),
                                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)restore_lds_bytes(32)));
        ctx->img->restore_lds_raised = true;
    }
    const dim3 grid((unsigned)((N + RS_TW - 1) / RS_TW), (unsigned)((N + RS_TH - 1) / RS_TH));
    hipLaunchKernelGGL(restore_kernel, grid, dim3(256), restore_lds_bytes(s), ctx->stream, N, model, residual, beam, s,
                       staged_stride(s), restored);
    GH_CHECK_HIP(ctx, hipGetLastError());
    return GRIDHIP_OK;
}

}  // namespace gridhip

using namespace gridhip;

namespace {

int fit_beam_any(gridhip_ctx *ctx, bool dev, int64_t N, const double *psf, int64_t window, double cut, double *beam)
{
    if (!ctx) return GRIDHIP_EINVAL;
    GH_CHECK(fit_beam_check(ctx, N, psf, window, cut, beam));
    GH_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    Staged st(ctx, dev);
    psf = st.in(psf, (size_t)N * N * 8), beam = st.out(beam, 64);
    GH_CHECK(st.status());
    GH_CHECK(fit_beam_run(ctx, N, psf, window, cut, beam));
    return st.finish();
}

int restore_any(gridhip_ctx *ctx, bool dev, int64_t N, const double *model, const double *residual, const double *beam,
                int64_t support, double *restored)
{
    if (!ctx) return GRIDHIP_EINVAL;
    GH_CHECK(restore_check(ctx, N, model, residual, beam, support, restored));
    if (!dev && !beam_usable(beam[0], beam[1], beam[2], beam[7]))
        return fail(ctx, GRIDHIP_EINVAL, "restore: the beam's fit failed, or A, B, C are not finite and positive definite");
    GH_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    const size_t bytes = (size_t)N * N * 8;
    Staged st(ctx, dev);
    model = st.in(model, bytes), restored = st.inout(residual, restored, bytes);
    if (!dev) residual = restored;  // (the staged residual is restored in place)
    beam = st.in(beam, 64);
    GH_CHECK(st.status());
    GH_CHECK(restore_run(ctx, N, model, residual, beam, support, restored));
    return st.finish();
}

}  // namespace

extern "C" {

int gridhip_fit_beam(gridhip_ctx *ctx, int64_t N, const double *psf, int64_t window, double cut, double *beam)
{
    return fit_beam_any(ctx, false, N, psf, window, cut, beam);
}

int gridhip_fit_beam_dev(gridhip_ctx *ctx, int64_t N, const double *psf, int64_t window, double cut, double *beam)
{
    return fit_beam_any(ctx, true, N, psf, window, cut, beam);
}

int gridhip_restore(gridhip_ctx *ctx, int64_t N, const double *model, const double *residual, const double *beam,
                    int64_t support, double *restored)
{
    return restore_any(ctx, false, N, model, residual, beam, support, restored);
}

int gridhip_restore_dev(gridhip_ctx *ctx, int64_t N, const double *model, const double *residual, const double *beam,
                        int64_t support, double *restored)
{
    return restore_any(ctx, true, N, model, residual, beam, support, restored);
}

}  // extern "C"
