// Multi-term CLEAN, the minor cycle of wide-band imaging (include/gridhip.h, "wide-band imaging"): T Taylor terms of the
// residual are cleaned together with the 2T - 1 spectral PSFs (Sault & Wieringa 1994; Rau & Cornwell 2011, one scale).
// The shape is clean.hip's: tiles of CLEAN_TH x CLEAN_TW, a device table of one (score, index) entry per tile, a state
// block that holds the stop condition, niter iterations enqueued unconditionally - and the code is: the walk over a tile,
// the table's reduction and the launch loop are clean_walk.h's; this file has what T terms add to them.  One call is
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
#include "clean_walk.h"

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

// What clean_tile_walk (clean_walk.h) does with T terms: T residual planes and 2T - 1 PSF planes, N * N cells apart;
// R_t loses the products f_q P_{t+q}, q ascending, each rounded, then subtracted; the score of a cell from its T values.
template <int TT>
struct MfWalk {
    static constexpr int T = TT, NP = 2 * TT - 1;
    double *res;
    const double *psf;
    int64_t cells;
    double f[TT], Hinv[TT * TT];
    __device__ __forceinline__ double product(int t, int q, const double (&p)[NP]) const
    {
#pragma clang fp contract(off)
        return f[q] * p[t + q];
    }
    __device__ __forceinline__ double score(const double (&r)[T]) const { return mf_score<T>(Hinv, r); }
    __device__ __forceinline__ bool searched(int64_t) const { return true; }
};

// One tile per work-group, clean_tile_kernel's geometry: SUB = false over all tiles, SUB = true over the tiles the update
// region can overlap, counted from its first tile.  The slots a lane takes are those of plane 0; for odd N the planes
// are 8 bytes apart in alignment, and the walk takes a plane (or a shifted PSF address) that is not aligned where plane 0
// is by two 8-byte accesses.
template <int T, bool SUB>
__global__ void __launch_bounds__(256)
    mf_tile_kernel(int64_t N, int64_t border, int64_t patch, int ntx, const double *__restrict__ psfs, double *res,
                   CleanEntry *__restrict__ table, const MfState *st)
{
    __shared__ CleanEntry sh[4];
    if (SUB && st->stopped) return;
    MfWalk<T> w;
    w.res = res, w.psf = psfs, w.cells = N * N;
    if (SUB) {
        for (int t = 0; t < T; ++t) w.f[t] = st->f[t];
        for (int i = 0; i < T * T; ++i) w.Hinv[i] = st->Hinv[i];
    } else {
        for (int t = 0; t < T; ++t) w.f[t] = 0.0;
        (void)mf_invert<T>(psfs, w.cells, (N / 2) * N + N / 2, w.Hinv);  // (a singular one: the first pick stops the call)
    }
    clean_tile_walk<SUB>(N, border, patch, ntx, SUB ? st->k : 0, table, sh, w);
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
    double bv;
    long long bk;
    table_best(table, ntiles, bv, bk, sh);
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

template <int T>
void mf_launch(gridhip_ctx *ctx, int64_t N, const double *psfs, double *res, double *models, double gain,
               double threshold, int64_t niter, int64_t border, int64_t patch, double *stats, void *scratch)
{
    const CleanTiles g = clean_tiles(N, patch);
    MfState *st = reinterpret_cast<MfState *>(scratch);
    CleanEntry *table = reinterpret_cast<CleanEntry *>(st + 1);
    const auto tile = [&](auto sub, const dim3 &grid) {
        hipLaunchKernelGGL((mf_tile_kernel<T, decltype(sub)::value>), grid, dim3(256), 0, ctx->stream, N, border, patch,
                           g.ntx, psfs, res, table, (const MfState *)st);
    };
    const auto pick = [&](auto init) {
        hipLaunchKernelGGL((mf_pick_kernel<T, decltype(init)::value>), dim3(1), dim3(1024), 0, ctx->stream, N, g.ntiles,
                           (const CleanEntry *)table, st, psfs, (const double *)res, models, gain, threshold, niter, stats);
    };
    clean_launch_loop(
        niter, [&] { tile(std::false_type{}, g.all); }, [&] { pick(std::true_type{}); },
        [&] { tile(std::true_type{}, g.part); }, [&] { pick(std::false_type{}); });
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
    return sizeof(MfState) + (size_t)clean_tiles(N).ntiles * sizeof(CleanEntry);
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
    const size_t plane = (size_t)N * N * 8, pb = (size_t)(2 * T - 1) * plane, rb = (size_t)T * plane;
    Staged st(ctx, dev);
    psfs = st.in(psfs, pb), residuals = st.inout(residuals, residuals, rb), models = st.inout(models, models, rb);
    stats = st.out(stats, 64);
    GH_CHECK(st.status());
    GH_CHECK(mfclean_run(ctx, N, T, psfs, residuals, models, gain, threshold, niter, border, patch, stats, scratch.p));
    return st.finish();
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
