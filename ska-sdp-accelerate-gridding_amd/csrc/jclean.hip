// Joint CLEAN (include/gridhip.h, "joint deconvolution"): P images of one sky - Stokes planes, channels - are searched on
// one combined statistic and every component is taken at one cell in all of them, each plane with its own peak value and
// its own (or the one shared) PSF.  The shape is mfclean.hip's: tiles of CLEAN_TH x CLEAN_TW, a device table of one
// (score, index) entry per tile, a state block that holds the stop condition, niter iterations enqueued unconditionally -
// and the code is clean_walk.h's: the walk over a tile, the table's reduction, the stop level and the launch loop; this
// file has the policy of P independent planes and its pick kernel.  One call is
//     j_tile_kernel<P, SHARED, false>   builds the table: one pass over the P residuals
//     j_pick_kernel<P, true>            computes the stop level from the first peak, starts the state, takes the first
//                                       component
//     niter x { j_tile_kernel<P, SHARED, true>   subtracts f_p * psf_q(p) from plane p over the update region and recomputes
//                                                the tiles' scores in the same pass
//               j_pick_kernel<P, false>          reduces the table, tests the stop rule, reads the P cells at the peak and
//                                                takes the next component }
// An iteration reads P residuals and Q PSFs and writes P residuals over the update region: (2P + Q) * 8 B per cell.  The
// kernels are templated on P and on SHARED (Q == 1) so that the 2P + Q values of a cell live in registers; the metric and
// the mask are wave-uniform branches.  No atomics; contraction is off: a plain restatement in numpy gives the same bits.
#include "common.h"
#include "clean_walk.h"

namespace gridhip {

namespace {

struct JState {  // 256 bytes at the head of the scratch block, the same for every P
    double f[JC_MAX_PLANES];     // gain * R_p[k] of the component the next tile kernel subtracts
    double flux[JC_MAX_PLANES];  // sums of the f_p added to the models
    double s;                    // the statistic at the current peak; NaN when no cell can be selected
    long long k;                 // its flat index, -1 when none
    long long iters;             // components taken so far
    long long stopped;           // every later launch returns
    long long reason;            // 0 niter taken, 1 stop level, 2 nothing selectable, 3 no usable sigma
    double L;                    // the stop level, in the statistic's units
    double s1;                   // the statistic at the first peak
    long long pad[9];
};
static_assert(sizeof(JState) == 256, "the state block's size is part of the scratch layout");

struct JSearch {  // what the search needs beside the residuals, by value in the launch
    double w[JC_MAX_PLANES];
    const uint8_t *mask;
    int metric;
};

// What clean_tile_walk (clean_walk.h) does with P independent planes: P residual planes and 1 (SHARED) or P PSF planes,
// N * N cells apart.  The update is diagonal: plane t loses f[t] * psf_q(t), the product rounded before the walk subtracts
// it, and nothing else - the products q != t are the constant +0.0, whose subtraction changes no bit of any value and is
// folded away where the walk's loops are unrolled (8 multiplications per cell for P = 8, not 64).  The score is
// w_0 * R_0^d + w_1 * R_1^d + ..., d = metric + 1, p ascending from the first term, every product rounded, then added.
template <int PP, bool SHARED>
struct JointWalk {
    static constexpr int T = PP, NP = SHARED ? 1 : PP;
    double *res;
    const double *psf;
    int64_t cells;
    double f[PP], w[PP];
    const uint8_t *mask;
    int metric;
    __device__ __forceinline__ double product(int t, int q, const double (&p)[NP]) const
    {
#pragma clang fp contract(off)
        return q == t ? f[t] * p[SHARED ? 0 : t] : 0.0;
    }
    __device__ __forceinline__ double score(const double (&r)[T]) const
    {
#pragma clang fp contract(off)
        double s;
        if (metric == 0) {
            s = w[0] * r[0];
#pragma unroll
            for (int t = 1; t < T; ++t) s = s + w[t] * r[t];
        } else {
            s = w[0] * (r[0] * r[0]);
#pragma unroll
            for (int t = 1; t < T; ++t) s = s + w[t] * (r[t] * r[t]);
        }
        return s;
    }
    __device__ __forceinline__ bool searched(int64_t a) const { return !mask || mask[a] != 0; }
};

// One tile per work-group, clean_tile_kernel's geometry: SUB = false over all tiles, SUB = true over the tiles the update
// region can overlap, counted from its first tile.
template <int P, bool SHARED, bool SUB>
__global__ void __launch_bounds__(256)
    j_tile_kernel(int64_t N, int64_t border, int64_t patch, int ntx, const double *__restrict__ psfs, double *res,
                  CleanEntry *__restrict__ table, const JState *st, const JSearch se)
{
    __shared__ CleanEntry sh[4];
    if (SUB && st->stopped) return;
    JointWalk<P, SHARED> w;
    w.res = res, w.psf = psfs, w.cells = N * N, w.mask = se.mask, w.metric = se.metric;
#pragma unroll
    for (int t = 0; t < P; ++t) w.f[t] = SUB ? st->f[t] : 0.0, w.w[t] = se.w[t];
    clean_tile_walk<SUB>(N, border, patch, ntx, SUB ? st->k : 0, table, sh, w);
}

// x^d, d = metric + 1: x itself, or x * x rounded once
__device__ __forceinline__ double j_pow(double x, int metric)
{
#pragma clang fp contract(off)
    return metric == 0 ? x : x * x;
}

// One work-group: the table's best is the cell with the largest |s|.  Then, by thread 0, the head of the next iteration:
// the stop rule - no usable sigma, nothing selectable, |s| <= L, niter components taken, before anything is subtracted -
// else the component: f_p = gain * R_p[k] into the state, where the next tile kernel finds it, and into models[p] and
// flux_p (one fused step each, as clean's).  INIT: the first pick of a call, which starts the state from zero and
// computes L = max(threshold^d, (nsigma * sigma)^d, peak_frac^d * |s1|) by stop_level's rule: the powers are taken here,
// and sigma's term goes in as 1.0 * (nsigma * sigma)^d, which is that value's own bits.
template <int P, bool INIT>
__global__ void __launch_bounds__(1024)
    j_pick_kernel(int64_t N, int ntiles, const CleanEntry *__restrict__ table, JState *st, const double *res,
                  double *models, int metric, double gain, double threshold, int64_t niter, double nsigma,
                  const double *noise, double peak_frac, double *stats)
{
#pragma clang fp contract(off)
    __shared__ CleanEntry sh[16];
    if (!INIT && st->stopped) return;
    double bv;
    long long bk;
    table_best(table, ntiles, bv, bk, sh);
    if (threadIdx.x != 0) return;
    const int64_t cells = N * N;
    double flux[P];
    long long iters = 0;
    for (int p = 0; p < P; ++p) flux[p] = INIT ? 0.0 : st->flux[p];
    if (!INIT) iters = st->iters;
    const double s = bk < 0 ? __builtin_nan("") : bv;
    bool bad = false;
    double L;
    if (INIT) {
        double a = 0.0;
        if (nsigma > 0.0) a = j_pow(nsigma * *noise, metric);
        L = stop_level(j_pow(threshold, metric), nsigma > 0.0 ? 1.0 : 0.0, &a, j_pow(peak_frac, metric), s, &bad);
    } else {
        L = st->L;
    }
    const bool stop = bad || bk < 0 || iters >= niter || !(fabs(bv) > L);
    if (!stop) {
        for (int p = 0; p < P; ++p) {
            const double R = res[p * cells + bk];
            st->f[p] = gain * R;
            models[p * cells + bk] = fma(gain, R, models[p * cells + bk]);
            flux[p] = fma(gain, R, flux[p]);
        }
        iters += 1;
    }
    const long long reason = !stop ? 0 : bad ? 3 : bk < 0 ? 2 : !(fabs(bv) > L) ? 1 : 0;
    st->s = s;
    st->k = bk;
    st->iters = iters;
    for (int p = 0; p < P; ++p) st->flux[p] = flux[p];
    st->stopped = stop ? 1 : 0;
    st->reason = reason;
    if (INIT) st->L = L, st->s1 = s;
    if (stats) {
        stats[0] = (double)iters;
        stats[1] = s;
        stats[2] = (double)bk;
        stats[4] = (double)reason;
        for (int p = 0; p < P; ++p) stats[8 + p] = flux[p];
        if (INIT) {
            stats[3] = L, stats[5] = s, stats[6] = 0.0, stats[7] = 0.0;
            for (int p = P; p < JC_MAX_PLANES; ++p) stats[8 + p] = 0.0;
        }
    }
}

struct JArgs {  // a checked call, as the launcher of every P takes it
    int64_t N;
    const double *psfs;
    double *res, *models;
    JSearch se;
    double gain, threshold;
    int64_t niter, border, patch;
    double nsigma;
    const double *noise;
    double peak_frac;
    double *stats;
    void *scratch;
};

template <int P, bool SHARED>
void j_launch(gridhip_ctx *ctx, const JArgs &a)
{
    const CleanTiles g = clean_tiles(a.N, a.patch);
    JState *st = reinterpret_cast<JState *>(a.scratch);
    CleanEntry *table = reinterpret_cast<CleanEntry *>(st + 1);
    const auto tile = [&](auto sub, const dim3 &grid) {
        hipLaunchKernelGGL((j_tile_kernel<P, SHARED, decltype(sub)::value>), grid, dim3(256), 0, ctx->stream, a.N, a.border,
                           a.patch, g.ntx, a.psfs, a.res, table, (const JState *)st, a.se);
    };
    const auto pick = [&](auto init) {
        hipLaunchKernelGGL((j_pick_kernel<P, decltype(init)::value>), dim3(1), dim3(1024), 0, ctx->stream, a.N, g.ntiles,
                           (const CleanEntry *)table, st, (const double *)a.res, a.models, a.se.metric, a.gain, a.threshold,
                           a.niter, a.nsigma, a.noise, a.peak_frac, a.stats);
    };
    clean_launch_loop(
        a.niter, [&] { tile(std::false_type{}, g.all); }, [&] { pick(std::true_type{}); },
        [&] { tile(std::true_type{}, g.part); }, [&] { pick(std::false_type{}); });
}

// (one plane has one PSF: P = 1 is the shared form alone)
template <int P>
void j_launch_planes(gridhip_ctx *ctx, bool shared, const JArgs &a)
{
    if constexpr (P > 1) {
        if (!shared) return j_launch<P, false>(ctx, a);
    }
    j_launch<P, true>(ctx, a);
}

}  // namespace

int jclean_check(gridhip_ctx *ctx, int64_t N, int64_t P, int64_t Q, const double *psfs, const double *residuals,
                 const double *models, const double *weights, int metric, double gain, double threshold, int64_t niter,
                 int64_t border, int64_t patch, const uint8_t *mask, double nsigma, const double *noise, double peak_frac)
{
    if (P < 1 || P > JC_MAX_PLANES) return fail(ctx, GRIDHIP_EINVAL, "jclean: P must be 1 to %d", JC_MAX_PLANES);
    if (Q != 1 && Q != P) return fail(ctx, GRIDHIP_EINVAL, "jclean: Q must be 1 or P");
    if (metric != 0 && metric != 1) return fail(ctx, GRIDHIP_EINVAL, "jclean: metric must be 0 (sum) or 1 (sumsq)");
    if (weights) {
        bool some = false;
        for (int64_t p = 0; p < P; ++p) {
            if (!(weights[p] >= 0.0 && weights[p] < __builtin_inf()))
                return fail(ctx, GRIDHIP_EINVAL, "jclean: a weight must be finite and >= 0");
            some = some || weights[p] > 0.0;
        }
        if (!some) return fail(ctx, GRIDHIP_EINVAL, "jclean: at least one weight must be > 0");
    }
    GH_CHECK(clean_check(ctx, N, psfs, residuals, models, gain, threshold, niter, border, patch));
    GH_CHECK(clean_auto_check(ctx, N, residuals, models, mask, nsigma, noise, peak_frac));
    const size_t plane = (size_t)N * N * 8, pb = (size_t)Q * plane, rb = (size_t)P * plane, mb = plane / 8;
    if (overlap(psfs, pb, residuals, rb) || overlap(psfs, pb, models, rb) || overlap(residuals, rb, models, rb) ||
        overlap(mask, mb, psfs, pb) || overlap(mask, mb, residuals, rb) || overlap(mask, mb, models, rb))
        return fail(ctx, GRIDHIP_EINVAL, "jclean: psfs, residuals, models and the mask must not overlap");
    return GRIDHIP_OK;
}

size_t jclean_scratch_bytes(int64_t N)
{
    return sizeof(JState) + (size_t)clean_tiles(N).ntiles * sizeof(CleanEntry);
}

int jclean_run(gridhip_ctx *ctx, int64_t N, int64_t P, int64_t Q, const double *psfs, double *residuals, double *models,
               const double *weights, int metric, double gain, double threshold, int64_t niter, int64_t border,
               int64_t patch, const uint8_t *mask, double nsigma, const double *noise, double peak_frac, double *stats,
               void *scratch)
{
    JArgs a{N, psfs, residuals, models, {}, gain, threshold, niter, border, patch, nsigma, noise, peak_frac, stats, scratch};
    for (int p = 0; p < JC_MAX_PLANES; ++p) a.se.w[p] = p >= P ? 0.0 : weights ? weights[p] : 1.0;
    a.se.mask = mask, a.se.metric = metric;
    const bool shared = Q == 1;
    switch (P) {
        case 1: j_launch_planes<1>(ctx, shared, a); break;
        case 2: j_launch_planes<2>(ctx, shared, a); break;
        case 3: j_launch_planes<3>(ctx, shared, a); break;
        case 4: j_launch_planes<4>(ctx, shared, a); break;
        case 5: j_launch_planes<5>(ctx, shared, a); break;
        case 6: j_launch_planes<6>(ctx, shared, a); break;
        case 7: j_launch_planes<7>(ctx, shared, a); break;
        default: j_launch_planes<8>(ctx, shared, a); break;
    }
    GH_CHECK_HIP(ctx, hipGetLastError());
    return GRIDHIP_OK;
}

}  // namespace gridhip

using namespace gridhip;

namespace {

int jclean_any(gridhip_ctx *ctx, bool dev, int64_t N, int64_t P, int64_t Q, const double *psfs, double *residuals,
               double *models, const double *weights, int metric, double gain, double threshold, int64_t niter,
               int64_t border, int64_t patch, const uint8_t *mask, double nsigma, const double *noise, double peak_frac,
               double *stats)
{
    if (!ctx) return GRIDHIP_EINVAL;
    GH_CHECK(jclean_check(ctx, N, P, Q, psfs, residuals, models, weights, metric, gain, threshold, niter, border, patch, mask,
                          nsigma, noise, peak_frac));
    GH_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    DevBuf scratch;
    GH_CHECK(scratch.alloc(ctx, jclean_scratch_bytes(N)));
    const size_t plane = (size_t)N * N * 8, rb = (size_t)P * plane;
    Staged st(ctx, dev);
    psfs = st.in(psfs, (size_t)Q * plane), residuals = st.inout(residuals, residuals, rb);
    models = st.inout(models, models, rb), stats = st.out(stats, 8 * GRIDHIP_JCLEAN_STATS), mask = st.in(mask, plane / 8);
    if (nsigma > 0.0) noise = st.in(noise, 8);
    GH_CHECK(st.status());
    GH_CHECK(jclean_run(ctx, N, P, Q, psfs, residuals, models, weights, metric, gain, threshold, niter, border, patch, mask,
                        nsigma, noise, peak_frac, stats, scratch.p));
    return st.finish();
}

}  // namespace

extern "C" {

int gridhip_jclean(gridhip_ctx *ctx, int64_t N, int64_t P, int64_t Q, const double *psfs, double *residuals, double *models,
                   const double *weights, int metric, double gain, double threshold, int64_t niter, int64_t border,
                   int64_t patch, const uint8_t *mask, double nsigma, const double *noise, double peak_frac, double *stats)
{
    return jclean_any(ctx, false, N, P, Q, psfs, residuals, models, weights, metric, gain, threshold, niter, border, patch,
                      mask, nsigma, noise, peak_frac, stats);
}

int gridhip_jclean_dev(gridhip_ctx *ctx, int64_t N, int64_t P, int64_t Q, const double *psfs, double *residuals,
                       double *models, const double *weights, int metric, double gain, double threshold, int64_t niter,
                       int64_t border, int64_t patch, const uint8_t *mask, double nsigma, const double *noise,
                       double peak_frac, double *stats)
{
    return jclean_any(ctx, true, N, P, Q, psfs, residuals, models, weights, metric, gain, threshold, niter, border, patch,
                      mask, nsigma, noise, peak_frac, stats);
}

}  // extern "C"
