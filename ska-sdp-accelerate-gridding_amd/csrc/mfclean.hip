// Multi-term CLEAN, the minor cycle of wide-band imaging (include/gridhip.h, "wide-band imaging"): T Taylor terms of the
// residual are cleaned together with the 2T - 1 spectral PSFs (Sault & Wieringa 1994; Rau & Cornwell 2011, one scale).
// The shape is clean.hip's: tiles of CLEAN_TH x CLEAN_TW, a device table of one (score, index) entry per tile, a state
// block that holds the stop condition, niter iterations enqueued unconditionally.  One call is
//     mf_tile_kernel<T, false>   builds the table: one pass over the T residuals; each work-group inverts the T x T
//                                Hessian for itself (at most 7 doubles read, a few dozen operations)
//     mf_pick_kernel<T, true>    inverts it once more into the state block, starts the state, takes the first component
//     niter x { mf_tile_kernel<T, true>   subtracts the T shifted PSF combinations from the tiles the update region
//                                         overlaps and recomputes their scores in the same pass
//               mf_pick_kernel<T, false>  reduces the table, recomputes the coefficients at the peak from the T residual
//                                         cells, tests the stop rule, takes the next component }
// An iteration reads T residuals and 2T - 1 PSFs and writes T residuals over the update region: (4T - 1) * 8 B per cell
// against Hogbom's 24.  The kernels are templated on T so that the T x T products and the 3T - 1 values of a cell live in
// registers.  No atomics; contraction is off: a plain restatement in numpy gives the same bits.
#include "common.h"
#include "imaging.h"

namespace gridhip {

namespace {

struct MfState {  // 256 bytes at the head of the scratch block, the same for every T
    double Hinv[16];    // the inverse Hessian, row-major T x T
    double f[4];        // gain * a_t of the component the next tile kernel subtracts
    double flux[4];     // sums of the f_t added to the models
    double a0;          // a_0 at the current peak; NaN when no cell can be selected
    long long k;        // its flat index, -1 when none
    long long iters;    // components taken so far
    long long stopped;  // every later launch returns
    long long reason;   // 0 niter taken, 1 threshold, 2 nothing selectable, 3 singular Hessian
    long long pad[3];
};
static_assert(sizeof(MfState) == 256, "the state block's size is part of the scratch layout");

// Hinv = the inverse of H[t][q] = P_{t+q}[c, c] by Gauss-Jordan without pivoting: rows in order, the pivot row divided
// by the pivot, then taken from every other row - the product rounded, then subtracted.  false: a pivot is not > 0.
template <int T>
__device__ __forceinline__ bool mf_invert(const double *__restrict__ psfs, int64_t cells, int64_t centre, double *Hinv)
{
#pragma clang fp contract(off)
    double d[2 * T - 1], A[T][T], B[T][T];
    for (int s = 0; s < 2 * T - 1; ++s) d[s] = psfs[s * cells + centre];
    for (int t = 0; t < T; ++t)
        for (int q = 0; q < T; ++q) A[t][q] = d[t + q], B[t][q] = t == q ? 1.0 : 0.0;
    bool ok = true;
#pragma unroll
    for (int i = 0; i < T; ++i) {
        const double piv = A[i][i];
        if (!(piv > 0.0)) ok = false;
#pragma unroll
        for (int j = 0; j < T; ++j) A[i][j] = A[i][j] / piv, B[i][j] = B[i][j] / piv;
#pragma unroll
        for (int r = 0; r < T; ++r) {
            if (r == i) continue;
            const double m = A[r][i];
#pragma unroll
            for (int j = 0; j < T; ++j) A[r][j] = A[r][j] - m * A[i][j], B[r][j] = B[r][j] - m * B[i][j];
        }
    }
    for (int t = 0; t < T; ++t)
        for (int q = 0; q < T; ++q) Hinv[t * T + q] = B[t][q];
    return ok;
}

// a_t = sum_q Hinv[t][q] * R_q, q ascending from the first product, each product rounded, then added
template <int T>
__device__ __forceinline__ void mf_coeffs(const double *Hinv, const double *R, double *a)
{
#pragma clang fp contract(off)
#pragma unroll
    for (int t = 0; t < T; ++t) {
        double s = Hinv[t * T] * R[0];
#pragma unroll
        for (int q = 1; q < T; ++q) s = s + Hinv[t * T + q] * R[q];
        a[t] = s;
    }
}

// s = sum_t a_t * R_t, likewise
template <int T>
__device__ __forceinline__ double mf_score(const double *Hinv, const double *R)
{
#pragma clang fp contract(off)
    double a[T];
    mf_coeffs<T>(Hinv, R, a);
    double s = a[0] * R[0];
#pragma unroll
    for (int t = 1; t < T; ++t) s = s + a[t] * R[t];
    return s;
}

// One tile per work-group, clean_tile_kernel's geometry: SUB = false over all tiles, SUB = true over the tiles the update
// region can overlap, counted from its first tile.  A lane takes the two cells of one 16-byte slot of the row, in all T
// residual planes and - inside the region - all 2T - 1 PSF planes; the slots are those of plane 0.  For odd N the planes
// are 8 bytes apart in alignment, so a plane (or a shifted PSF address) that is not aligned where plane 0 is takes its
// two cells by two 8-byte accesses.
template <int T, bool SUB>
__global__ void __launch_bounds__(256)
    mf_tile_kernel(int64_t N, int64_t border, int64_t patch, int ntx, const double *__restrict__ psfs, double *res,
                   CleanEntry *__restrict__ table, const MfState *st)
{
#pragma clang fp contract(off)
    __shared__ CleanEntry sh[4];
    int64_t tx = blockIdx.x, ty = blockIdx.y;
    int64_t ylo = 0, yhi = -1, xlo = 0, xhi = -1, py = 0, px = 0;
    const int64_t c = N / 2, cells = N * N;
    double f[T], Hinv[T * T];
    if (SUB) {
        if (st->stopped) return;
        const int64_t k = st->k;
        for (int t = 0; t < T; ++t) f[t] = st->f[t];
        for (int i = 0; i < T * T; ++i) Hinv[i] = st->Hinv[i];
        py = k / N, px = k % N;
        ylo = py - c, yhi = py - c + N - 1, xlo = px - c, xhi = px - c + N - 1;
        if (patch > 0) {
            ylo = hi64(ylo, py - patch), yhi = lo64(yhi, py + patch);
            xlo = hi64(xlo, px - patch), xhi = lo64(xhi, px + patch);
        }
        ylo = hi64(ylo, 0), yhi = lo64(yhi, N - 1), xlo = hi64(xlo, 0), xhi = lo64(xhi, N - 1);
        ty += ylo / CLEAN_TH, tx += xlo / CLEAN_TW;
        if (ty > yhi / CLEAN_TH || tx > xhi / CLEAN_TW) return;
    } else {
        for (int t = 0; t < T; ++t) f[t] = 0.0;
        (void)mf_invert<T>(psfs, cells, c * N + c, Hinv);  // (a singular one: the first pick stops the call)
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t x0 = tx * CLEAN_TW, x1 = lo64(x0 + CLEAN_TW, N);
    const int64_t mis = (int64_t)(((uintptr_t)res >> 3) & 1);  // res + a is 16-byte aligned where a + mis is even
    double bv = 0.0;
    long long bk = -1;
    for (int r = wave; r < CLEAN_TH; r += 4) {
        const int64_t y = ty * CLEAN_TH + r;
        if (y >= N) break;
        const int64_t base = y * N;
        const bool yin = SUB && y >= ylo && y <= yhi, ysearch = y >= border && y < N - border;
        const int64_t poff = (y - py + c) * N + (c - px) - base;  // psf index of the cell at flat index a: a + poff
        const int64_t a0 = ((base + x0 + mis) & ~(int64_t)1) - mis, a1 = base + x1;
        for (int64_t a = a0 + 2 * lane; a < a1; a += 128) {
            const int64_t x = a - base;
            const bool v0 = x >= x0, v1 = x + 1 < x1;  // (at least one holds: a slot has a cell of this tile's row)
            double r0[T], r1[T];
#pragma unroll
            for (int t = 0; t < T; ++t) {
                const double *q = res + t * cells + a;
                r0[t] = 0.0, r1[t] = 0.0;
                if (v0 && v1 && ((uintptr_t)q & 15) == 0) {
                    const double2 w = *reinterpret_cast<const double2 *>(q);
                    r0[t] = w.x, r1[t] = w.y;
                } else {
                    if (v0) r0[t] = q[0];
                    if (v1) r1[t] = q[1];
                }
            }
            if (yin) {
                const bool u0 = v0 && x >= xlo && x <= xhi, u1 = v1 && x + 1 >= xlo && x + 1 <= xhi;
                if (u0 || u1) {
                    double p0[2 * T - 1], p1[2 * T - 1];
#pragma unroll
                    for (int s = 0; s < 2 * T - 1; ++s) {
                        const double *q = psfs + s * cells + (a + poff);
                        p0[s] = 0.0, p1[s] = 0.0;
                        if (u0 && u1 && ((uintptr_t)q & 15) == 0) {
                            const double2 w = *reinterpret_cast<const double2 *>(q);
                            p0[s] = w.x, p1[s] = w.y;
                        } else {
                            if (u0) p0[s] = q[0];
                            if (u1) p1[s] = q[1];
                        }
                    }
#pragma unroll
                    for (int t = 0; t < T; ++t) {
#pragma unroll
                        for (int q = 0; q < T; ++q) {
                            if (u0) r0[t] = r0[t] - f[q] * p0[t + q];
                            if (u1) r1[t] = r1[t] - f[q] * p1[t + q];
                        }
                        double *o = res + t * cells + a;
                        if (u0 && u1 && ((uintptr_t)o & 15) == 0) {
                            *reinterpret_cast<double2 *>(o) = make_double2(r0[t], r1[t]);
                        } else {
                            if (u0) o[0] = r0[t];
                            if (u1) o[1] = r1[t];
                        }
                    }
                }
            }
            if (ysearch) {
                if (v0 && x >= border && x < N - border) consider(mf_score<T>(Hinv, r0), a, bv, bk);
                if (v1 && x + 1 >= border && x + 1 < N - border) consider(mf_score<T>(Hinv, r1), a + 1, bv, bk);
            }
        }
    }
    group_best(bv, bk, sh);
    if (threadIdx.x == 0) table[ty * ntx + tx] = {bv, bk};
}

// One work-group: the table's best is the cell with the largest score.  Then, by thread 0, the head of the next
// iteration: the coefficients a_t at that cell from the T residual cells, the stop rule on p = a_0 - nothing selectable,
// niter components taken, |p| <= threshold, before anything is subtracted - else the component: f_t = gain * a_t into
// the state, where the next tile kernel finds it, and into models[t] and flux_t (one fused step each, as clean's).
// INIT: the first pick of a call, which inverts the Hessian into the state and starts the state from zero.
template <int T, bool INIT>
__global__ void __launch_bounds__(1024)
    mf_pick_kernel(int64_t N, int ntiles, const CleanEntry *__restrict__ table, MfState *st,
                   const double *__restrict__ psfs, const double *res, double *models, double gain, double threshold,
                   int64_t niter, double *stats)
{
#pragma clang fp contract(off)
    __shared__ CleanEntry sh[16];
    if (!INIT && st->stopped) return;
    double bv = 0.0;
    long long bk = -1;
    for (int t = threadIdx.x; t < ntiles; t += blockDim.x) consider(table[t].v, table[t].k, bv, bk);
    group_best(bv, bk, sh);
    if (threadIdx.x != 0) return;
    const int64_t cells = N * N;
    double Hinv[T * T], flux[4] = {0.0, 0.0, 0.0, 0.0};
    long long iters = 0;
    bool singular = false;
    if (INIT) {
        singular = !mf_invert<T>(psfs, cells, (N / 2) * N + N / 2, Hinv);
        for (int i = 0; i < T * T; ++i) st->Hinv[i] = Hinv[i];
    } else {
        for (int i = 0; i < T * T; ++i) Hinv[i] = st->Hinv[i];
        for (int t = 0; t < T; ++t) flux[t] = st->flux[t];
        iters = st->iters;
    }
    if (singular) bk = -1;
    double a[T], p = __builtin_nan("");
    if (bk >= 0) {
        double R[T];
        for (int t = 0; t < T; ++t) R[t] = res[t * cells + bk];
        mf_coeffs<T>(Hinv, R, a);
        p = a[0];
    }
    const bool stop = singular || bk < 0 || iters >= niter || !(fabs(p) > threshold);
    if (!stop) {
        for (int t = 0; t < T; ++t) {
            st->f[t] = gain * a[t];
            models[t * cells + bk] = fma(gain, a[t], models[t * cells + bk]);
            flux[t] = fma(gain, a[t], flux[t]);
        }
        iters += 1;
    }
    const long long reason = !stop ? 0 : singular ? 3 : bk < 0 ? 2 : !(fabs(p) > threshold) ? 1 : 0;
    st->a0 = p;
    st->k = bk;
    st->iters = iters;
    for (int t = 0; t < 4; ++t) st->flux[t] = flux[t];
    st->stopped = stop ? 1 : 0;
    st->reason = reason;
    if (stats) {
        stats[0] = (double)iters;
        stats[1] = p;
        stats[2] = (double)bk;
        for (int t = 0; t < 4; ++t) stats[3 + t] = flux[t];
        stats[7] = (double)reason;
    }
}

bool overlap(const double *a, size_t abytes, const double *b, size_t bbytes)
{
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + bbytes && y < x + abytes;
}

template <int T>
void mf_launch(gridhip_ctx *ctx, int64_t N, const double *psfs, double *res, double *models, double gain,
               double threshold, int64_t niter, int64_t border, int64_t patch, double *stats, void *scratch)
{
    const int64_t ntx = (N + CLEAN_TW - 1) / CLEAN_TW, nty = (N + CLEAN_TH - 1) / CLEAN_TH;
    MfState *st = reinterpret_cast<MfState *>(scratch);
    CleanEntry *table = reinterpret_cast<CleanEntry *>(st + 1);
    const int ntiles = (int)(ntx * nty);
    const int64_t span = patch > 0 && 2 * patch + 1 < N ? 2 * patch + 1 : N;
    const dim3 all((unsigned)ntx, (unsigned)nty);
    const dim3 part((unsigned)tiles_spanned(span, CLEAN_TW, ntx), (unsigned)tiles_spanned(span, CLEAN_TH, nty));
    hipLaunchKernelGGL((mf_tile_kernel<T, false>), all, dim3(256), 0, ctx->stream, N, border, patch, (int)ntx, psfs, res,
                       table, (const MfState *)st);
    hipLaunchKernelGGL((mf_pick_kernel<T, true>), dim3(1), dim3(1024), 0, ctx->stream, N, ntiles,
                       (const CleanEntry *)table, st, psfs, (const double *)res, models, gain, threshold, niter, stats);
    for (int64_t i = 0; i < niter; ++i) {
        hipLaunchKernelGGL((mf_tile_kernel<T, true>), part, dim3(256), 0, ctx->stream, N, border, patch, (int)ntx, psfs, res,
                           table, (const MfState *)st);
        hipLaunchKernelGGL((mf_pick_kernel<T, false>), dim3(1), dim3(1024), 0, ctx->stream, N, ntiles,
                           (const CleanEntry *)table, st, psfs, (const double *)res, models, gain, threshold, niter, stats);
    }
}

}  // namespace

int mfclean_check(gridhip_ctx *ctx, int64_t N, int64_t T, const double *psfs, const double *residuals,
                  const double *models, double gain, double threshold, int64_t niter, int64_t border, int64_t patch)
{
    if (T < 1 || T > MF_MAX_TERMS) return fail(ctx, GRIDHIP_EINVAL, "mfclean: T must be 1 to %d", MF_MAX_TERMS);
    GH_CHECK(clean_check(ctx, N, psfs, residuals, models, gain, threshold, niter, border, patch));
    const size_t plane = (size_t)N * N * 8, pb = (size_t)(2 * T - 1) * plane, rb = (size_t)T * plane;
    if (overlap(psfs, pb, residuals, rb) || overlap(psfs, pb, models, rb) || overlap(residuals, rb, models, rb))
        return fail(ctx, GRIDHIP_EINVAL, "mfclean: psfs, residuals and models must not overlap");
    return GRIDHIP_OK;
}

size_t mfclean_scratch_bytes(int64_t N)
{
    const int64_t ntx = (N + CLEAN_TW - 1) / CLEAN_TW, nty = (N + CLEAN_TH - 1) / CLEAN_TH;
    return sizeof(MfState) + (size_t)ntx * nty * sizeof(CleanEntry);
}

int mfclean_run(gridhip_ctx *ctx, int64_t N, int64_t T, const double *psfs, double *residuals, double *models,
                double gain, double threshold, int64_t niter, int64_t border, int64_t patch, double *stats, void *scratch)
{
    switch (T) {
        case 1: mf_launch<1>(ctx, N, psfs, residuals, models, gain, threshold, niter, border, patch, stats, scratch); break;
        case 2: mf_launch<2>(ctx, N, psfs, residuals, models, gain, threshold, niter, border, patch, stats, scratch); break;
        case 3: mf_launch<3>(ctx, N, psfs, residuals, models, gain, threshold, niter, border, patch, stats, scratch); break;
        default: mf_launch<4>(ctx, N, psfs, residuals, models, gain, threshold, niter, border, patch, stats, scratch); break;
    }
    GH_CHECK_HIP(ctx, hipGetLastError());
    return GRIDHIP_OK;
}

}  // namespace gridhip

using namespace gridhip;

namespace {

int mfclean_any(gridhip_ctx *ctx, bool dev, int64_t N, int64_t T, const double *psfs, double *residuals, double *models,
                double gain, double threshold, int64_t niter, int64_t border, int64_t patch, double *stats)
{
    if (!ctx) return GRIDHIP_EINVAL;
    GH_CHECK(mfclean_check(ctx, N, T, psfs, residuals, models, gain, threshold, niter, border, patch));
    GH_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    DevBuf scratch;
    GH_CHECK(scratch.alloc(ctx, mfclean_scratch_bytes(N)));
    if (dev)
        return mfclean_run(ctx, N, T, psfs, residuals, models, gain, threshold, niter, border, patch, stats, scratch.p);
    const size_t plane = (size_t)N * N * 8, pb = (size_t)(2 * T - 1) * plane, rb = (size_t)T * plane;
    DevBuf p, r, m, s;
    GH_CHECK(p.upload(ctx, psfs, pb));
    GH_CHECK(r.upload(ctx, residuals, rb));
    GH_CHECK(m.upload(ctx, models, rb));
    GH_CHECK(s.alloc(ctx, 64));
    GH_CHECK(mfclean_run(ctx, N, T, p.as<double>(), r.as<double>(), m.as<double>(), gain, threshold, niter, border, patch,
                         s.as<double>(), scratch.p));
    GH_CHECK(d2h(ctx, residuals, r.p, rb));
    GH_CHECK(d2h(ctx, models, m.p, rb));
    if (stats) GH_CHECK(d2h(ctx, stats, s.p, 64));
    return sync(ctx);
}

}  // namespace

extern "C" {

int gridhip_mfclean(gridhip_ctx *ctx, int64_t N, int64_t T, const double *psfs, double *residuals, double *models,
                    double gain, double threshold, int64_t niter, int64_t border, int64_t patch, double *stats)
{
    return mfclean_any(ctx, false, N, T, psfs, residuals, models, gain, threshold, niter, border, patch, stats);
}

int gridhip_mfclean_dev(gridhip_ctx *ctx, int64_t N, int64_t T, const double *psfs, double *residuals, double *models,
                        double gain, double threshold, int64_t niter, int64_t border, int64_t patch, double *stats)
{
    return mfclean_any(ctx, true, N, T, psfs, residuals, models, gain, threshold, niter, border, patch, stats);
}

}  // extern "C"
