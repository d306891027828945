// Antenna-gain self-calibration (include/gridhip.h, "gain calibration"): scalar gains per (solution interval, antenna) by
// StEFCal, and their application to a visibility stream.  Everything stays on the device: the stop condition lives in a
// small state block, the host enqueues niter iterations unconditionally and reads nothing back, and a launch whose state
// is stopped returns at its first instruction (clean.hip's scheme).
//
//     gaincal_init_kernel     the [T][A][3] table, the solved flags start from zero, the gains from 1 (a kernel: no memset node)
//     gaincal_prepare_kernel  one pass over V, M, s, a1, a2, slot: X (16 B), Y (8 B) and the packed 8-byte key per
//                             visibility, and the sums that do not depend on the gains (chi^2 at g = 1, used, flagged,
//                             dropped) - one row of partial sums per work-group, no atomics
//     gaincal_begin_kernel    one work-group adds the rows in a fixed order and starts the state block (gain_common.h,
//                             with everything else ddcal.hip and jonescal.hip share: the key, the state block, the classes,
//                             the products, the interval walk gc_walk, the driver gc_solve_run and the entry gc_solve_any)
//     niter x { gaincal_iter_kernel    streams key, X, Y (32 B per visibility).  A work-group takes a contiguous range of
//                                      whole chunks of GC_CHUNK visibilities, keeps the gains and a (num.re, num.im, den)
//                                      accumulator of ONE interval in LDS (A <= GC_LDS_A: 16 A + 24 A bytes, 20 KB at
//                                      A = 512; its registers leave GC_RESIDENT such work-groups per CU), adds with LDS
//                                      fp64 atomics and flushes to the global table with global fp64 atomics when the interval changes
//                                      and at the end of its range.  A time-major stream changes interval a few times per
//                                      range; an unordered one is still right - it flushes per change and is slower.
//                                      A > GC_LDS_A: gaincal_iter_global_kernel adds to the global table directly.
//               gaincal_update_kernel  one work-group: g' from the table, the phase-only and averaging rules, rel in a
//                                      fixed order, the stop test; zeroes the table for the next iteration }
//     gc_finish_kernel        (gain_common.h) one work-group: the reference-antenna rotation and the number of unsolved (t, a)
//     gaincal_stream_kernel   one pass over the visibilities with the final gains: chi^2 (partial rows), and - selfcal -
//                             the corrected visibilities and weights in the same pass; alone it is gridhip_apply_gains
//     gaincal_stats_kernel    one work-group adds the chi^2 rows in a fixed order and writes the 8 doubles (gain_common.h)
// The rotation is not fused into the streaming pass: the pass reads gains of every antenna of an interval, so the rotated
// table must be complete before it starts, and a kernel boundary is the only grid-wide ordering used anywhere here.
// Determinism: the table's sums meet in fp64 atomics (LDS, then global), so gains agree to the order of those sums and not
// bit for bit; rel, chi^2 and the counts are added in a fixed order given the gains.  Contraction is off where the header
// names the rounding (X, Y).
#include "gain_common.h"

namespace gridhip {

namespace {

// work-groups of gaincal_iter_kernel resident on a CU: the kernel takes 84 VGPRs, which the hardware allocates as 88, so a
// SIMD holds 512 / 88 = 5 waves and a CU five work-groups of four waves (LDS, 20.3 KB each, would allow seven)
constexpr int GC_RESIDENT = 5;
constexpr int GC_BLOCK = 256;  // its work-group: a step of the walk is 4 visibilities per thread
static_assert(GC_CHUNK % (4 * GC_BLOCK) == 0, "a chunk is whole steps");

// cells: T * A.  The table (3 doubles per cell) and the flags (one 32-bit word per cell) are zeroed; warm: the gains stay
__global__ void __launch_bounds__(256)
    gaincal_init_kernel(int64_t cells, int warm, double *__restrict__ table, unsigned int *__restrict__ ever,
                        double2 *__restrict__ g)
{
    const int64_t k0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, step = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = k0; e < cells; e += step) {
        table[3 * e] = 0.0, table[3 * e + 1] = 0.0, table[3 * e + 2] = 0.0;
        ever[e] = 0u;
        if (!warm) g[e] = make_double2(1.0, 0.0);
    }
}

__global__ void __launch_bounds__(256)
    gaincal_prepare_kernel(int64_t n, int64_t A, int64_t T, const int64_t *__restrict__ a1, const int64_t *__restrict__ a2,
                           const int64_t *__restrict__ slot, const double2 *__restrict__ vis,
                           const double2 *__restrict__ mod, const double *__restrict__ wt, double2 *__restrict__ X,
                           double *__restrict__ Y, unsigned long long *__restrict__ key, double *__restrict__ parts)
{
#pragma clang fp contract(off)
    __shared__ double lds[16];
    const int64_t k0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, step = (int64_t)gridDim.x * blockDim.x;
    double chi0 = 0.0;
    unsigned int used = 0, flagged = 0, dropped = 0;  // (a lane sees far fewer than 2^32 visibilities)
    for (int64_t k = k0; k < n; k += step) {
        int64_t p, q, t;
        double s;
        const int c = classify(k, A, T, a1, a2, slot, wt, &p, &q, &t, &s);
        used += c == 0, flagged += c == 1, dropped += c == 2;
        double2 x = make_double2(0.0, 0.0);
        double y = 0.0;
        unsigned long long kk = 0ull;
        if (c == 0) {
            const double2 v = vis[k], m = mod[k];
            x = cmulc(make_double2(s * v.x, s * v.y), m);
            y = s * norm2(m);
            const double2 r = make_double2(v.x - m.x, v.y - m.y);
            chi0 += s * norm2(r);
            kk = gc_pack(p, q, t);
        }
        X[k] = x, Y[k] = y, key[k] = kk;
    }
    gc_prepare_tail(chi0, used, flagged, dropped, parts, lds);
}

// What gc_walk needs of this module.  A lane loads X and Y of its four visibilities (32 B each) at the start of a step,
// before the interval loop; the add is the two sides' (num.re, num.im, den).  GcSolve below adds the driver's part.
struct GcMod {
    static constexpr int NS = 3, NG = 1, GSTEP = 1, UNROLL = 4;
    struct In {
        const double2 *X;
        const double *Y;
    };
    struct Held {
        double2 x[4];
        double y[4];
        __device__ __forceinline__ void load(const In &in, int j, int64_t k, bool there)
        {
            x[j] = there ? in.X[k] : make_double2(0.0, 0.0);
            y[j] = there ? in.Y[k] : 0.0;
        }
    };
    static __device__ __forceinline__ void load_gains(double2 *lg, const double2 *__restrict__ g, long long tn, int A, int64_t)
    {
        gc_copy_gains(lg, g, tn, A);
    }
    static __device__ __forceinline__ void add(const In &, const Held &h, int j, int64_t, const double2 *gp,
                                               const double2 *gq, int64_t, double *rp, double *rq)
    {
        const double2 x = h.x[j], a = *gp, b = *gq;
        const double y = h.y[j];
        const double2 np = cmul(x, b), nq = cmul(make_double2(x.x, -x.y), a);
        atomicAdd(&rp[0], np.x), atomicAdd(&rp[1], np.y), atomicAdd(&rp[2], y * norm2(b));
        atomicAdd(&rq[0], nq.x), atomicAdd(&rq[1], nq.y), atomicAdd(&rq[2], y * norm2(a));
    }
};

// One iteration's sums, A <= GC_LDS_A: gc_walk with static LDS, 16 A + 24 A bytes
__global__ void __launch_bounds__(GC_BLOCK)
    gaincal_iter_kernel(int64_t n, int A, int64_t per, const double2 *__restrict__ X, const double *__restrict__ Y,
                        const unsigned long long *__restrict__ key, const double2 *__restrict__ g, double *table,
                        const GcState *st)
{
    __shared__ double2 lg[GC_LDS_A];
    __shared__ double acc[3 * GC_LDS_A];
    gc_walk<GcMod>(GcMod::In{X, Y}, n, A, 1, per, key, g, table, st, lg, acc);
}

__global__ void __launch_bounds__(256)
    gaincal_iter_global_kernel(int64_t n, int64_t A, const double2 *__restrict__ X, const double *__restrict__ Y,
                               const unsigned long long *__restrict__ key, const double2 *__restrict__ g, double *table,
                               const GcState *st)
{
    gc_walk_global<GcMod>(GcMod::In{X, Y}, n, A, 1, key, g, table, st);
}

// One work-group of 1024 threads: thread i takes the cells i, i + 1024, ... in order.  The phase-only rule applies where
// the cell was solved in this iteration: an unsolved gain stays the bits it was.
__global__ void __launch_bounds__(1024)
    gaincal_update_kernel(int64_t cells, int mode, double tol, double *__restrict__ table, unsigned int *__restrict__ ever,
                          double2 *__restrict__ g, GcState *st)
{
#pragma clang fp contract(off)
    if (st->stopped) return;
    __shared__ double lds[16];
    const bool odd = (st->iters & 1) != 0;
    double d2 = 0.0, s2 = 0.0;
    for (int64_t e = threadIdx.x; e < cells; e += 1024) {
        const double nr = table[3 * e], ni = table[3 * e + 1], den = table[3 * e + 2];
        table[3 * e] = 0.0, table[3 * e + 1] = 0.0, table[3 * e + 2] = 0.0;
        const double2 go = g[e];
        double2 gn = go;
        if (den > 0.0) {
            ever[e] = 1u;
            gn = make_double2(nr / den, ni / den);
            if (mode == 1) {
                const double a = sqrt(norm2(gn));
                gn = a > 0.0 ? make_double2(gn.x / a, gn.y / a) : go;
            }
            if (odd) gn = make_double2((gn.x + go.x) / 2.0, (gn.y + go.y) / 2.0);
            g[e] = gn;
        }
        d2 += norm2(make_double2(gn.x - go.x, gn.y - go.y));
        s2 += norm2(gn);
    }
    gc_close_iteration(d2, s2, tol, st, lds);
}

// What gridhip_apply_gains does with one visibility (include/gridhip.h): returns the output weight
__device__ __forceinline__ double apply_one(bool inrange, double2 gp, double2 gq, int inverse, double2 v, double s,
                                            double2 *out)
{
#pragma clang fp contract(off)
    if (!inrange) {
        *out = v;
        return inverse ? 0.0 : s;
    }
    if (!inverse) {
        *out = cmulc(cmul(gp, v), gq);
        return s;
    }
    const double np = norm2(gp), nq = norm2(gq);
    if (!(np > 0.0 && nq > 0.0 && np - np == 0.0 && nq - nq == 0.0)) {  // a gain that is zero or not finite
        *out = v;
        return 0.0;
    }
    const double2 d = cmulc(gp, gq), num = cmulc(v, d);
    const double dd = norm2(d);
    *out = make_double2(num.x / dd, num.y / dd);
    return s * np * nq;
}

// One pass with the final gains.  CHI: the partial sums of chi^2 over the used visibilities (vis against mod), one per
// work-group.  APPLY: vout, wout (may be null) = apply_gains(vis, wt); they may be vis and wt themselves (element k is read
// before it is written, by the same lane): no __restrict__ on those.
template <bool CHI, bool APPLY>
__global__ void __launch_bounds__(256)
    gaincal_stream_kernel(int64_t n, int64_t A, int64_t T, const int64_t *__restrict__ a1, const int64_t *__restrict__ a2,
                          const int64_t *__restrict__ slot, const double2 *__restrict__ g, const double2 *vis,
                          const double2 *__restrict__ mod, const double *wt, int inverse, double2 *vout, double *wout,
                          double *__restrict__ parts)
{
#pragma clang fp contract(off)
    __shared__ double lds[16];
    const int64_t k0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, step = (int64_t)gridDim.x * blockDim.x;
    double chi = 0.0;
    for (int64_t k = k0; k < n; k += step) {
        const double s = wt ? wt[k] : 1.0;
        const int64_t p = a1[k], q = a2[k], t = slot ? slot[k] : 0;
        const bool inrange = p >= 0 && p < A && q >= 0 && q < A && t >= 0 && t < T;
        double2 gp = make_double2(1.0, 0.0), gq = gp;
        if (inrange) gp = g[t * A + p], gq = g[t * A + q];
        const double2 v = vis[k];
        if (CHI && inrange && p != q && s > 0.0) {
            const double2 m = cmulc(cmul(gp, mod[k]), gq);
            chi += s * norm2(make_double2(v.x - m.x, v.y - m.y));
        }
        if (APPLY) {
            double2 o;
            const double w = apply_one(inrange, gp, gq, inverse, v, s, &o);
            vout[k] = o;
            if (wout) wout[k] = w;
        }
    }
    if (CHI) {
        chi = block_sum(chi, lds);
        if (threadIdx.x == 0) parts[blockIdx.x] = chi;
    }
}

// what gc_solve_run and gc_solve_any need of this module: a fixed work-group of GC_BLOCK with static LDS, its launches
struct GcSolve : GcMod {
    static constexpr int BLOCK = GC_BLOCK, RESIDENT = GC_RESIDENT, LDS_MOST = 0, RAISE_BIT = 0;
    static constexpr bool PAIR = true;  // X
    static const void *walker() { return nullptr; }
    static int64_t lds_antennas() { return GC_LDS_A; }
    static GcPlanes planes(const GcCall &c) { return {1, c.A * c.T, 1, true, 0u}; }
    static GcRules rules(const GcCall &c) { return {"gaincal", 1, false, 16, 16, (size_t)c.A * c.T * 16}; }
    static int run(gridhip_ctx *ctx, const GcCall &c) { return gc_solve_run<GcSolve>(ctx, c); }
    static void init(gridhip_ctx *ctx, const GcCall &c, const GcWork &w)
    {
        hipLaunchKernelGGL(gaincal_init_kernel, grid_for(ctx, c.A * c.T), dim3(256), 0, ctx->stream, c.A * c.T, c.warm,
                           w.table, w.ever, w.g);
    }
    static void prepare(gridhip_ctx *ctx, const GcCall &c, const GcWork &w)
    {
        hipLaunchKernelGGL(gaincal_prepare_kernel, w.sgrid, dim3(256), 0, ctx->stream, c.n, c.A, c.T, c.a1, c.a2, c.slot,
                           (const double2 *)c.vis, (const double2 *)c.model_vis, c.wt, w.pair, w.real, w.key, w.parts);
    }
    static void iter(gridhip_ctx *ctx, const GcCall &c, const GcWork &w, bool lds, dim3 grid, dim3 block, size_t,
                     int64_t per)
    {
        if (lds)
            hipLaunchKernelGGL(gaincal_iter_kernel, grid, block, 0, ctx->stream, c.n, (int)c.A, per, (const double2 *)w.pair,
                               (const double *)w.real, (const unsigned long long *)w.key, (const double2 *)w.g, w.table,
                               (const GcState *)w.st);
        else
            hipLaunchKernelGGL(gaincal_iter_global_kernel, w.sgrid, dim3(256), 0, ctx->stream, c.n, c.A,
                               (const double2 *)w.pair, (const double *)w.real, (const unsigned long long *)w.key,
                               (const double2 *)w.g, w.table, (const GcState *)w.st);
    }
    static void update(gridhip_ctx *ctx, const GcCall &c, const GcWork &w)
    {
        hipLaunchKernelGGL(gaincal_update_kernel, dim3(1), dim3(1024), 0, ctx->stream, c.A * c.T, c.mode, c.tol, w.table,
                           w.ever, w.g, w.st);
    }
    static void final(gridhip_ctx *ctx, const GcCall &c, const GcWork &w)  // a selfcal: the corrected stream in the same pass
    {
        const auto pass = c.vis_cal ? gaincal_stream_kernel<true, true> : gaincal_stream_kernel<true, false>;
        hipLaunchKernelGGL(pass, w.sgrid, dim3(256), 0, ctx->stream, c.n, c.A, c.T, c.a1, c.a2, c.slot, (const double2 *)w.g,
                           (const double2 *)c.vis, (const double2 *)c.model_vis, c.wt, 1, (double2 *)c.vis_cal,
                           c.vis_cal ? c.wt_cal : nullptr, w.parts);
    }
};

}  // namespace

int gaincal_check(gridhip_ctx *ctx, int64_t n, int64_t A, int64_t T, const int64_t *a1, const int64_t *a2,
                  const int64_t *slot, const double *vis, const double *model_vis, const double *wt, int mode,
                  int64_t refant, int64_t niter, double tol, const double *gains)
{
    const GcCall c = {n, A, T, 1, a1, a2, slot, vis, model_vis, wt, mode, refant, 0, niter, tol, const_cast<double *>(gains)};
    return gc_solve_check(ctx, GcSolve::rules(c), c);
}

int apply_gains_check(gridhip_ctx *ctx, int64_t n, int64_t A, int64_t T, const int64_t *a1, const int64_t *a2,
                      const int64_t *slot, const double *gains, int inverse, const double *vis_in, const double *wt_in,
                      const double *vis_out, const double *wt_out)
{
    if (n < 0 || A < 2 || T < 1 || (!slot && T != 1) || (n > 0 && (!a1 || !a2 || !vis_in || !vis_out)) || !gains ||
        inverse < 0 || inverse > 1)
        return fail(ctx, GRIDHIP_EINVAL, "apply_gains: bad argument");
    GH_CHECK(shape_check(ctx, "apply_gains", n, A, T, a1, a2, slot));
    const size_t gb = (size_t)A * T * 16, n8 = (size_t)n * 8;
    const Range vo = {vis_out, 2 * n8}, wo = {wt_out, n8};
    if (overlaps_any(vo, {{gains, gb}, {a1, n8}, {a2, n8}, {slot, n8}}) ||
        overlaps_any(wo, {{gains, gb}, {a1, n8}, {a2, n8}, {slot, n8}}))
        return fail(ctx, GRIDHIP_EINVAL, "apply_gains: an output overlaps gains, a1, a2 or slot");
    // in place: vis_out may be vis_in itself and wt_out may be wt_in itself, nothing else
    // (both outputs against the inputs before one against the other: which message a doubly wrong call gets)
    if (outputs_clash({vo}, {{vis_in, 2 * n8}, {wt_in, n8}}, {{0, 0}}) ||
        outputs_clash({wo}, {{vis_in, 2 * n8}, {wt_in, n8}}, {{0, 1}}))
        return fail(ctx, GRIDHIP_EINVAL, "apply_gains: an output may be its own input, and overlap no other");
    if (overlap(vo.p, vo.bytes, wo.p, wo.bytes)) return fail(ctx, GRIDHIP_EINVAL, "apply_gains: vis_out overlaps wt_out");
    return GRIDHIP_OK;
}

int apply_gains_run(gridhip_ctx *ctx, int64_t n, int64_t A, int64_t T, const int64_t *a1, const int64_t *a2,
                    const int64_t *slot, const double *gains, int inverse, const double *vis_in, const double *wt_in,
                    double *vis_out, double *wt_out)
{
    if (n == 0) return GRIDHIP_OK;
    hipLaunchKernelGGL((gaincal_stream_kernel<false, true>), grid_for(ctx, n), dim3(256), 0, ctx->stream, n, A, T, a1, a2,
                       slot, (const double2 *)gains, (const double2 *)vis_in, (const double2 *)nullptr, wt_in, inverse,
                       (double2 *)vis_out, wt_out, (double *)nullptr);
    GH_CHECK_HIP(ctx, hipGetLastError());
    return GRIDHIP_OK;
}

int gaincal_run(gridhip_ctx *ctx, int64_t n, int64_t A, int64_t T, const int64_t *a1, const int64_t *a2,
                const int64_t *slot, const double *vis, const double *model_vis, const double *wt, int mode, int64_t refant,
                int warm, int64_t niter, double tol, double *gains, double *stats, double *vis_cal, double *wt_cal)
{
    return GcSolve::run(ctx, {n, A, T, 1, a1, a2, slot, vis, model_vis, wt, mode, refant, warm, niter, tol, gains, stats,
                              vis_cal, wt_cal});
}

}  // namespace gridhip

using namespace gridhip;

namespace {

int apply_gains_any(gridhip_ctx *ctx, bool dev, int64_t n, int64_t A, int64_t T, const int64_t *a1, const int64_t *a2,
                    const int64_t *slot, const double *gains, int inverse, const double *vis_in, const double *wt_in,
                    double *vis_out, double *wt_out)
{
    if (!ctx) return GRIDHIP_EINVAL;
    GH_CHECK(apply_gains_check(ctx, n, A, T, a1, a2, slot, gains, inverse, vis_in, wt_in, vis_out, wt_out));
    GH_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n8 = (size_t)n * 8;
    Staged st(ctx, dev);
    a1 = st.in(a1, n8), a2 = st.in(a2, n8), slot = st.in(slot, n8), gains = st.in(gains, (size_t)A * T * 16);
    vis_out = st.inout(vis_in, vis_out, 2 * n8);
    if (!dev) vis_in = vis_out;  // (the staged visibilities are corrected in place)
    wt_in = st.in(wt_in, n8), wt_out = st.out(wt_out, n8);
    GH_CHECK(st.status());
    GH_CHECK(apply_gains_run(ctx, n, A, T, a1, a2, slot, gains, inverse, vis_in, wt_in, vis_out, wt_out));
    return st.finish();
}

}  // namespace

extern "C" {

int gridhip_gaincal_dev(gridhip_ctx *ctx, int64_t n, int64_t A, int64_t T, const int64_t *a1, const int64_t *a2,
                        const int64_t *slot, const double *vis, const double *model_vis, const double *wt, int mode,
                        int64_t refant, int warm, int64_t niter, double tol, double *gains, double *stats)
{
    return gc_solve_any<GcSolve>(ctx, true, {n, A, T, 1, a1, a2, slot, vis, model_vis, wt, mode, refant, warm, niter, tol,
                                             gains, stats});
}

int gridhip_gaincal(gridhip_ctx *ctx, int64_t n, int64_t A, int64_t T, const int64_t *a1, const int64_t *a2,
                    const int64_t *slot, const double *vis, const double *model_vis, const double *wt, int mode,
                    int64_t refant, int warm, int64_t niter, double tol, double *gains, double *stats)
{
    return gc_solve_any<GcSolve>(ctx, false, {n, A, T, 1, a1, a2, slot, vis, model_vis, wt, mode, refant, warm, niter, tol,
                                              gains, stats});
}

int gridhip_apply_gains_dev(gridhip_ctx *ctx, int64_t n, int64_t A, int64_t T, const int64_t *a1, const int64_t *a2,
                            const int64_t *slot, const double *gains, int inverse, const double *vis_in,
                            const double *wt_in, double *vis_out, double *wt_out)
{
    return apply_gains_any(ctx, true, n, A, T, a1, a2, slot, gains, inverse, vis_in, wt_in, vis_out, wt_out);
}

int gridhip_apply_gains(gridhip_ctx *ctx, int64_t n, int64_t A, int64_t T, const int64_t *a1, const int64_t *a2,
                        const int64_t *slot, const double *gains, int inverse, const double *vis_in, const double *wt_in,
                        double *vis_out, double *wt_out)
{
    return apply_gains_any(ctx, false, n, A, T, a1, a2, slot, gains, inverse, vis_in, wt_in, vis_out, wt_out);
}

}  // extern "C"
