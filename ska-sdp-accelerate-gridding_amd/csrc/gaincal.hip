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
//                             with everything else ddcal.hip shares: the key, the state block, the classes, the products)
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
//     gaincal_finish_kernel   one work-group: the reference-antenna rotation and the number of unsolved (t, a)
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

// work-groups of gaincal_iter_kernel resident on a CU: the kernel takes 82 VGPRs, which the hardware allocates as 88, so a
// SIMD holds 512 / 88 = 5 waves and a CU five work-groups of four waves (LDS, 20.3 KB each, would allow seven)
constexpr int GC_RESIDENT = 5;
constexpr int GC_STEP = 1024;  // visibilities a work-group takes between two barriers: 4 per thread
static_assert(GC_CHUNK % GC_STEP == 0, "a chunk is whole steps");

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
            kk = GC_USED | (unsigned long long)p | (unsigned long long)q << 21 | (unsigned long long)t << 42;
        }
        X[k] = x, Y[k] = y, key[k] = kk;
    }
    const double r[GC_PARTS] = {chi0, (double)used, (double)flagged, (double)dropped};
    for (int j = 0; j < GC_PARTS; ++j) {
        const double x = block_sum(r[j], lds);
        if (threadIdx.x == 0) parts[(int64_t)blockIdx.x * GC_PARTS + j] = x;
    }
}

// One iteration's sums, A <= GC_LDS_A.  Work-group b takes the visibilities [b * per, (b + 1) * per), per a whole number
// of chunks, in steps of GC_STEP: thread i holds the visibilities base + i + 256 j.  lg, acc: the gains and the sums of
// interval tcur.  A step whose used visibilities all lie in tcur costs one barrier; otherwise the work-group agrees on the
// lowest interval still pending, flushes, loads that interval's gains and goes on until nothing is pending.
__global__ void __launch_bounds__(256)
    gaincal_iter_kernel(int64_t n, int A, int64_t per, const double2 *__restrict__ X, const double *__restrict__ Y,
                        const unsigned long long *__restrict__ key, const double2 *__restrict__ g, double *table,
                        const GcState *st)
{
    if (st->stopped) return;
    __shared__ double2 lg[GC_LDS_A];
    __shared__ double acc[3 * GC_LDS_A];
    __shared__ unsigned int tsel;
    for (int a = threadIdx.x; a < 3 * A; a += 256) acc[a] = 0.0;
    const int64_t k0 = (int64_t)blockIdx.x * per, k1 = k0 + per < n ? k0 + per : n;
    long long tcur = -1;
    for (int64_t base = k0; base < k1; base += GC_STEP) {
        unsigned long long kk[4];
        double2 x[4];
        double y[4];
        unsigned int pend = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t k = base + threadIdx.x + 256 * j;
            kk[j] = 0ull, x[j] = make_double2(0.0, 0.0), y[j] = 0.0;
            if (k < k1) {
                kk[j] = key[k];
                x[j] = X[k];
                y[j] = Y[k];
            }
            if (kk[j] & GC_USED) pend |= 1u << j;
        }
        for (;;) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (!(pend >> j & 1u) || (long long)(kk[j] >> 42 & GC_FIELD) != tcur) continue;
                const int p = (int)(kk[j] & GC_FIELD), q = (int)(kk[j] >> 21 & GC_FIELD);
                const double2 gp = lg[p], gq = lg[q];
                const double2 np = cmul(x[j], gq), nq = cmul(make_double2(x[j].x, -x[j].y), gp);
                atomicAdd(&acc[3 * p], np.x), atomicAdd(&acc[3 * p + 1], np.y), atomicAdd(&acc[3 * p + 2], y[j] * norm2(gq));
                atomicAdd(&acc[3 * q], nq.x), atomicAdd(&acc[3 * q + 1], nq.y), atomicAdd(&acc[3 * q + 2], y[j] * norm2(gp));
                pend &= ~(1u << j);
            }
            if (!__syncthreads_or(pend != 0)) break;  // (a barrier: every add into tcur's sums is done)
            if (threadIdx.x == 0) tsel = 0xffffffffu;
            __syncthreads();
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (pend >> j & 1u) atomicMin(&tsel, (unsigned int)(kk[j] >> 42 & GC_FIELD));
            __syncthreads();
            const long long tn = tsel;
            for (int a = threadIdx.x; a < A; a += 256) {
                if (tcur >= 0) {
                    double *row = table + 3 * (tcur * A + a);
                    for (int c = 0; c < 3; ++c) {
                        const double v = acc[3 * a + c];
                        if (v != 0.0) atomicAdd(&row[c], v);
                        acc[3 * a + c] = 0.0;
                    }
                }
                lg[a] = g[tn * A + a];
            }
            __syncthreads();
            tcur = tn;
        }
    }
    __syncthreads();
    if (tcur >= 0)
        for (int a = threadIdx.x; a < A; a += 256) {
            double *row = table + 3 * (tcur * A + a);
            for (int c = 0; c < 3; ++c) {
                const double v = acc[3 * a + c];
                if (v != 0.0) atomicAdd(&row[c], v);
            }
        }
}

// the same sums for any A: gains from global memory, fp64 atomics straight to the table
__global__ void __launch_bounds__(256)
    gaincal_iter_global_kernel(int64_t n, int64_t A, const double2 *__restrict__ X, const double *__restrict__ Y,
                               const unsigned long long *__restrict__ key, const double2 *__restrict__ g, double *table,
                               const GcState *st)
{
    if (st->stopped) return;
    const int64_t k0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, step = (int64_t)gridDim.x * blockDim.x;
    for (int64_t k = k0; k < n; k += step) {
        const unsigned long long kk = key[k];
        if (!(kk & GC_USED)) continue;
        const int64_t t = (int64_t)(kk >> 42 & GC_FIELD), p = t * A + (int64_t)(kk & GC_FIELD),
                      q = t * A + (int64_t)(kk >> 21 & GC_FIELD);
        const double2 x = X[k], gp = g[p], gq = g[q];
        const double y = Y[k];
        const double2 np = cmul(x, gq), nq = cmul(make_double2(x.x, -x.y), gp);
        atomicAdd(&table[3 * p], np.x), atomicAdd(&table[3 * p + 1], np.y), atomicAdd(&table[3 * p + 2], y * norm2(gq));
        atomicAdd(&table[3 * q], nq.x), atomicAdd(&table[3 * q + 1], nq.y), atomicAdd(&table[3 * q + 2], y * norm2(gp));
    }
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
    d2 = block_sum(d2, lds);
    s2 = block_sum(s2, lds);
    if (threadIdx.x != 0) return;
    const double rel = sqrt(d2 / s2);
    st->rel = rel;
    st->iters += 1;
    if (tol > 0.0 && rel <= tol) st->stopped = 1;
}

// One work-group of 1024 threads.  rot[t] = conj(g[t, refant]) / |g[t, refant]| where the reference antenna was solved and
// its gain is finite and not zero, else 1: every solved gain of the interval is multiplied by it (an unsolved one stays
// exactly what it started from), the reference antenna's own becomes (|g|, 0).  The gains of an interval are read (rot) before any is written: a barrier lies between.
__global__ void __launch_bounds__(1024)
    gaincal_finish_kernel(int64_t A, int64_t T, int64_t refant, const unsigned int *__restrict__ ever, double2 *g,
                          double2 *__restrict__ rot, GcState *st)
{
#pragma clang fp contract(off)
    __shared__ double lds[16];
    if (refant >= 0) {
        for (int64_t t = threadIdx.x; t < T; t += 1024) {
            const double2 r = g[t * A + refant];
            const double a = sqrt(norm2(r));
            rot[t] = (ever[t * A + refant] && a > 0.0 && a - a == 0.0) ? make_double2(r.x / a, -r.y / a)
                                                                      : make_double2(1.0, 0.0);
        }
        __syncthreads();
    }
    double un = 0.0;
    for (int64_t e = threadIdx.x; e < A * T; e += 1024) {
        if (!ever[e]) {  // unsolved: counted, and the gain stays the bits it started from
            un += 1.0;
            continue;
        }
        if (refant < 0) continue;
        const int64_t t = e / A;
        const double2 r = rot[t];
        if (r.x == 1.0 && r.y == 0.0) continue;
        const double2 go = g[e];
        g[e] = e - t * A == refant ? make_double2(sqrt(norm2(go)), 0.0) : cmul(go, r);
    }
    un = block_sum(un, lds);
    if (threadIdx.x == 0) st->unsolved = (long long)un;
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

}  // namespace

int gaincal_check(gridhip_ctx *ctx, int64_t n, int64_t A, int64_t T, const int64_t *a1, const int64_t *a2,
                  const int64_t *slot, const double *vis, const double *model_vis, const double *wt, int mode,
                  int64_t refant, int64_t niter, double tol, const double *gains)
{
    if (n < 0 || A < 2 || T < 1 || (!slot && T != 1) || (n > 0 && (!a1 || !a2 || !vis || !model_vis)) || !gains ||
        niter < 0 || !(tol >= 0.0) || mode < 0 || mode > 1 || refant >= A)
        return fail(ctx, GRIDHIP_EINVAL, "gaincal: bad argument");
    GH_CHECK(shape_check(ctx, "gaincal", n, A, T, a1, a2, slot));
    const size_t gb = (size_t)A * T * 16, n8 = (size_t)n * 8;
    if (overlaps_any({gains, gb}, {{a1, n8}, {a2, n8}, {slot, n8}, {vis, 2 * n8}, {model_vis, 2 * n8}, {wt, n8}}))
        return fail(ctx, GRIDHIP_EINVAL, "gaincal: gains must not overlap an input");
    return GRIDHIP_OK;
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
    const int64_t cells = A * T;
    const dim3 sgrid = grid_for(ctx, n);  // the prepare pass and the final pass: one row of partial sums per work-group
    DevBuf small, table, ever, X, Y, key;
    GH_CHECK(small.alloc(ctx, ((size_t)GC_HEAD + (size_t)GC_PARTS * ctx->num_cu * 16 + 2 * (size_t)T) * 8));
    GH_CHECK(table.alloc(ctx, (size_t)cells * 24));
    GH_CHECK(ever.alloc(ctx, (size_t)cells * 4));
    if (n > 0) {
        GH_CHECK(X.alloc(ctx, (size_t)n * 16));
        GH_CHECK(Y.alloc(ctx, (size_t)n * 8));
        GH_CHECK(key.alloc(ctx, (size_t)n * 8));
    }
    GcState *st = small.as<GcState>();
    double *parts = small.as<double>() + GC_HEAD;
    double2 *rot = reinterpret_cast<double2 *>(parts + (size_t)GC_PARTS * ctx->num_cu * 16);
    double2 *g = (double2 *)gains;
    hipLaunchKernelGGL(gaincal_init_kernel, grid_for(ctx, cells), dim3(256), 0, ctx->stream, cells, warm, table.as<double>(),
                       ever.as<unsigned int>(), g);
    if (n > 0)
        hipLaunchKernelGGL(gaincal_prepare_kernel, sgrid, dim3(256), 0, ctx->stream, n, A, T, a1, a2, slot,
                           (const double2 *)vis, (const double2 *)model_vis, wt, X.as<double2>(), Y.as<double>(),
                           key.as<unsigned long long>(), parts);
    hipLaunchKernelGGL(gaincal_begin_kernel, dim3(1), dim3(256), 0, ctx->stream, n > 0 ? (int)sgrid.x : 0,
                       (const double *)parts, st);
    // the iteration kernel's ranges: whole chunks, GC_RESIDENT work-groups per CU at the most, so that every work-group
    // of the launch is resident at once and none waits for another to retire
    const int64_t nchunks = (n + GC_CHUNK - 1) / GC_CHUNK, most = (int64_t)ctx->num_cu * GC_RESIDENT;
    const int64_t cpw = nchunks > most ? (nchunks + most - 1) / most : 1;
    const int64_t igrid = nchunks > 0 ? (nchunks + cpw - 1) / cpw : 0;
    for (int64_t i = 0; i < niter; ++i) {
        if (n > 0 && A <= GC_LDS_A)
            hipLaunchKernelGGL(gaincal_iter_kernel, dim3((unsigned)igrid), dim3(256), 0, ctx->stream, n, (int)A,
                               cpw * GC_CHUNK, (const double2 *)X.as<double2>(), (const double *)Y.as<double>(),
                               (const unsigned long long *)key.as<unsigned long long>(), (const double2 *)g,
                               table.as<double>(), (const GcState *)st);
        else if (n > 0)
            hipLaunchKernelGGL(gaincal_iter_global_kernel, sgrid, dim3(256), 0, ctx->stream, n, A,
                               (const double2 *)X.as<double2>(), (const double *)Y.as<double>(),
                               (const unsigned long long *)key.as<unsigned long long>(), (const double2 *)g,
                               table.as<double>(), (const GcState *)st);
        hipLaunchKernelGGL(gaincal_update_kernel, dim3(1), dim3(1024), 0, ctx->stream, cells, mode, tol, table.as<double>(),
                           ever.as<unsigned int>(), g, st);
    }
    hipLaunchKernelGGL(gaincal_finish_kernel, dim3(1), dim3(1024), 0, ctx->stream, A, T, refant,
                       (const unsigned int *)ever.as<unsigned int>(), g, rot, st);
    if (n > 0) {
        if (vis_cal)
            hipLaunchKernelGGL((gaincal_stream_kernel<true, true>), sgrid, dim3(256), 0, ctx->stream, n, A, T, a1, a2, slot,
                               (const double2 *)g, (const double2 *)vis, (const double2 *)model_vis, wt, 1,
                               (double2 *)vis_cal, wt_cal, parts);
        else
            hipLaunchKernelGGL((gaincal_stream_kernel<true, false>), sgrid, dim3(256), 0, ctx->stream, n, A, T, a1, a2, slot,
                               (const double2 *)g, (const double2 *)vis, (const double2 *)model_vis, wt, 1,
                               (double2 *)nullptr, (double *)nullptr, parts);
    }
    if (stats)
        hipLaunchKernelGGL(gaincal_stats_kernel, dim3(1), dim3(256), 0, ctx->stream, n > 0 ? (int)sgrid.x : 0,
                           (const double *)parts, (const GcState *)st, stats);
    GH_CHECK_HIP(ctx, hipGetLastError());
    return GRIDHIP_OK;
}

}  // namespace gridhip

using namespace gridhip;

namespace {

int gaincal_any(gridhip_ctx *ctx, bool dev, int64_t n, int64_t A, int64_t T, const int64_t *a1, const int64_t *a2,
                const int64_t *slot, const double *vis, const double *model_vis, const double *wt, int mode, int64_t refant,
                int warm, int64_t niter, double tol, double *gains, double *stats)
{
    if (!ctx) return GRIDHIP_EINVAL;
    GH_CHECK(gaincal_check(ctx, n, A, T, a1, a2, slot, vis, model_vis, wt, mode, refant, niter, tol, gains));
    GH_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n8 = (size_t)n * 8, gb = (size_t)A * T * 16;
    Staged st(ctx, dev);
    a1 = st.in(a1, n8), a2 = st.in(a2, n8), slot = st.in(slot, n8), vis = st.in(vis, 2 * n8);
    model_vis = st.in(model_vis, 2 * n8), wt = st.in(wt, n8);
    gains = warm ? st.inout(gains, gains, gb) : st.out(gains, gb);  // (a cold start reads no gains)
    stats = st.out(stats, 64);
    GH_CHECK(st.status());
    GH_CHECK(gaincal_run(ctx, n, A, T, a1, a2, slot, vis, model_vis, wt, mode, refant, warm, niter, tol, gains, stats, nullptr,
                         nullptr));
    return st.finish();
}

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
    return gaincal_any(ctx, true, n, A, T, a1, a2, slot, vis, model_vis, wt, mode, refant, warm, niter, tol, gains, stats);
}

int gridhip_gaincal(gridhip_ctx *ctx, int64_t n, int64_t A, int64_t T, const int64_t *a1, const int64_t *a2,
                    const int64_t *slot, const double *vis, const double *model_vis, const double *wt, int mode,
                    int64_t refant, int warm, int64_t niter, double tol, double *gains, double *stats)
{
    return gaincal_any(ctx, false, n, A, T, a1, a2, slot, vis, model_vis, wt, mode, refant, warm, niter, tol, gains, stats);
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
