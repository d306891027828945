// Direction-dependent gain calibration (include/gridhip.h, "direction-dependent calibration"): D gain sets per (solution
// interval, antenna) by the multi-direction StEFCal, and the subtraction of corrupted directions from a visibility stream.
// The scheme is gaincal.hip's - the stop condition lives in the state block, niter iterations are enqueued unconditionally
// and a launch whose state is stopped returns at its first instruction - with a D x D normal matrix per (t, a) in place
// of one ratio, and what is the same in words is gain_common.h's: the interval walk, the driver, the entry point.
//
//     ddcal_init_kernel      the [T][A][D^2 + 2 D] table and the solved flags start from zero, the gains from 1
//     ddcal_prepare_kernel   one pass over V, M, s, a1, a2, slot: s V (16 B), s (8 B) and the packed 8-byte key per
//                            visibility, and the sums that do not depend on the gains (chi^2 at g = 1, the counts)
//     gaincal_begin_kernel   (gain_common.h) adds the rows in a fixed order and starts the state block
//     niter x { ddcal_iter_kernel<D>   streams key, s V, s and the D model values (32 + 16 D bytes per visibility).  A
//                                      work-group takes a contiguous range of whole chunks of GC_CHUNK visibilities and
//                                      keeps, for ONE interval, the gains (2 D doubles) and the sums (D real diagonals,
//                                      D (D - 1) / 2 complex entries of the upper triangle of H, D complex entries of b:
//                                      D^2 + 2 D doubles) of every antenna in LDS - (D^2 + 4 D) * 8 bytes per antenna,
//                                      dynamic, at most DD_LDS_BUDGET.  It adds with LDS fp64 atomics and flushes to the
//                                      global table with global fp64 atomics when the interval changes and at the end of
//                                      its range.  A > gridhip_ddcal_lds_antennas(D): ddcal_iter_global_kernel<D> adds
//                                      to the global table directly.
//               ddcal_solve_kernel<D>  one work-group: thread i takes the cells i, i + 512, ...: LDL^H in direction
//                                      order, the pivot rule, the phase-only and averaging rules, rel in a fixed order,
//                                      the stop test; zeroes the table for the next iteration }
//     gc_finish_kernel       (gain_common.h) one work-group: the rotation per direction and interval, the unsolved (t, a)
//     ddcal_chi_kernel       one pass with the final gains: chi^2 against the full sum over the directions
//     gaincal_stats_kernel   (gain_common.h) the 8 doubles
//     dd_subtract_kernel     vis_out = vis_in - the corrupted models of the chosen directions, one pass
// Occupancy of the iteration kernel: its work-groups are sized so that a CU holds 1024 threads whatever the table takes -
// four work-groups of 256 while four tables fit in the CU's 160 KB of LDS, two of 512, or one of 1024 once a table is above
// 80 KB - because a work-group alone on its CU with 256 threads would leave three quarters of the wave slots empty.
// Determinism: as gaincal.hip - the table's sums meet in fp64 atomics, everything after them is added in a fixed order.
#include "gain_common.h"

namespace gridhip {

namespace {

__host__ __device__ constexpr int dd_sums(int D) { return D * D + 2 * D; }  // doubles of H's upper triangle and b

// cells: T * A.  The table and the flags are zeroed; warm: the gains stay
__global__ void __launch_bounds__(256)
    ddcal_init_kernel(int64_t cells, int D, int warm, double *__restrict__ table, unsigned int *__restrict__ ever,
                      double2 *__restrict__ g)
{
    const int64_t k0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, step = (int64_t)gridDim.x * blockDim.x;
    const int64_t words = cells * dd_sums(D);
    for (int64_t e = k0; e < words; e += step) table[e] = 0.0;
    for (int64_t e = k0; e < cells; e += step) ever[e] = 0u;
    if (!warm)
        for (int64_t e = k0; e < cells * D; e += step) g[e] = make_double2(1.0, 0.0);
}

__global__ void __launch_bounds__(256)
    ddcal_prepare_kernel(int64_t n, int64_t A, int64_t T, int D, const int64_t *__restrict__ a1,
                         const int64_t *__restrict__ a2, const int64_t *__restrict__ slot, const double2 *__restrict__ vis,
                         const double2 *__restrict__ mod, const double *__restrict__ wt, double2 *__restrict__ sV,
                         double *__restrict__ S, unsigned long long *__restrict__ key, double *__restrict__ parts)
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
        unsigned long long kk = 0ull;
        if (c == 0) {
            const double2 v = vis[k];
            double2 r = v;
            for (int d = 0; d < D; ++d) {
                const double2 m = mod[(int64_t)d * n + k];
                r = make_double2(r.x - m.x, r.y - m.y);
            }
            x = make_double2(s * v.x, s * v.y);
            chi0 += s * norm2(r);
            kk = gc_pack(p, q, t);
        }
        sV[k] = x, S[k] = c == 0 ? s : 0.0, key[k] = kk;
    }
    gc_prepare_tail(chi0, used, flagged, dropped, parts, lds);
}

// One side of one visibility into the sums of its antenna: row = { H[d,d] (D), H[d,e] d < e row by row (re, im), b[d] (re,
// im) }, z the D regressors, s the weight, sy = s y.  H[d,e] += conj(z_d) (s z_e), b[d] += conj(z_d) (s y).
template <int D>
__device__ __forceinline__ void dd_add(double *row, const double2 (&z)[D], double s, double2 sy)
{
#pragma clang fp contract(off)
    int c = D;
#pragma unroll
    for (int d = 0; d < D; ++d) {
        atomicAdd(&row[d], (s * z[d].x) * z[d].x + (s * z[d].y) * z[d].y);
#pragma unroll
        for (int e = d + 1; e < D; ++e) {
            const double2 h = cmulc(make_double2(s * z[e].x, s * z[e].y), z[d]);
            atomicAdd(&row[c], h.x), atomicAdd(&row[c + 1], h.y);
            c += 2;
        }
        const double2 b = cmulc(sy, z[d]);
        atomicAdd(&row[D * D + 2 * d], b.x), atomicAdd(&row[D * D + 2 * d + 1], b.y);
    }
}

// both sides of visibility k, one after the other so that only one antenna's gains are held at a time: gp, gq point at
// the gains of its two antennas (direction d at gp[d * gstride]), rp, rq at their rows of sums
template <int D>
__device__ __forceinline__ void dd_visibility(int64_t n, int64_t k, const double2 *__restrict__ sV,
                                              const double *__restrict__ S, const double2 *__restrict__ M,
                                              const double2 *gp, const double2 *gq, int64_t gstride, double *rp, double *rq)
{
#pragma clang fp contract(off)
    const double2 sv = sV[k];
    const double s = S[k];
    double2 m[D], z[D];
#pragma unroll
    for (int d = 0; d < D; ++d) m[d] = M[(int64_t)d * n + k];
#pragma unroll
    for (int d = 0; d < D; ++d) z[d] = cmulc(m[d], gq[d * gstride]);  // M conj(g_q)
    dd_add<D>(rp, z, s, sv);
#pragma unroll
    for (int d = 0; d < D; ++d) {  // conj(M) conj(g_p)
        const double2 h = gp[d * gstride];
        z[d] = make_double2(m[d].x * h.x - m[d].y * h.y, -(m[d].x * h.y + m[d].y * h.x));
    }
    dd_add<D>(rq, z, s, make_double2(sv.x, -sv.y));
}

// What gc_walk needs of this module: lg [A][D] from the caller's [D][T][A], acc [A][D^2 + 2 D].  D > 3: one visibility at a
// time - unrolled, the loads of all four are hoisted together and the lane spills.  DdSolve<D> below adds the driver's part.
template <int D>
struct DdMod {
    static constexpr int NS = dd_sums(D), NG = D, GSTEP = 1, UNROLL = D > 3 ? 1 : 4;
    struct In {
        int64_t n;
        const double2 *sV;
        const double *S;
        const double2 *M;
    };
    using Held = GcNoHeld;
    static __device__ __forceinline__ void load_gains(double2 *lg, const double2 *__restrict__ g, long long tn, int A, int64_t T)
    {
        for (int a = threadIdx.x, nt = blockDim.x; a < D * A; a += nt) lg[a] = g[((int64_t)(a % D) * T + tn) * A + a / D];
    }
    static __device__ __forceinline__ void add(const In &in, const Held &, int, int64_t k, const double2 *gp,
                                               const double2 *gq, int64_t gstride, double *rp, double *rq)
    {
        dd_visibility<D>(in.n, k, in.sV, in.S, in.M, gp, gq, gstride, rp, rq);
    }
};

// One iteration's sums, A <= gridhip_ddcal_lds_antennas(D): gc_walk with dynamic LDS, (D^2 + 4 D) * 8 bytes per antenna
template <int D>
__global__ void __launch_bounds__(1024)
    ddcal_iter_kernel(int64_t n, int A, int64_t T, int64_t per, const double2 *__restrict__ sV, const double *__restrict__ S,
                      const unsigned long long *__restrict__ key, const double2 *__restrict__ M,
                      const double2 *__restrict__ g, double *table, const GcState *st)
{
    extern __shared__ double2 dd_lds[];
    gc_walk<DdMod<D>>(typename DdMod<D>::In{n, sV, S, M}, n, A, T, per, key, g, table, st, dd_lds,
                      reinterpret_cast<double *>(dd_lds + (size_t)D * A));
}

template <int D>
__global__ void __launch_bounds__(256)
    ddcal_iter_global_kernel(int64_t n, int64_t A, int64_t T, const double2 *__restrict__ sV, const double *__restrict__ S,
                             const unsigned long long *__restrict__ key, const double2 *__restrict__ M,
                             const double2 *__restrict__ g, double *table, const GcState *st)
{
    gc_walk_global<DdMod<D>>(typename DdMod<D>::In{n, sV, S, M}, n, A, T, key, g, table, st);
}

// One work-group of 512 threads: thread i takes the cells i, i + 512, ... in order.  H = L diag(dj) L^H with L unit lower
// triangular, in direction order and without pivoting; the cell is solved iff every dj > 1e-12 H[j,j].  An unsolved cell
// keeps the bits of all its D gains.
template <int D>
__global__ void __launch_bounds__(512)
    ddcal_solve_kernel(int64_t cells, int mode, double tol, double *__restrict__ table, unsigned int *__restrict__ ever,
                       double2 *__restrict__ g, GcState *st)
{
#pragma clang fp contract(off)
    if (st->stopped) return;
    __shared__ double lds[16];
    constexpr int NS = dd_sums(D);
    const bool odd = (st->iters & 1) != 0;
    double d2 = 0.0, s2 = 0.0;
    for (int64_t e = threadIdx.x; e < cells; e += 512) {
        double *row = table + e * NS;
        double hd[D], dj[D];
        double2 hu[D][D], L[D][D], b[D], x[D], go[D];  // hu[d][e], d < e: H[d,e];  L[i][j], i > j
        int c = D;
#pragma unroll
        for (int d = 0; d < D; ++d) hd[d] = row[d];
#pragma unroll
        for (int d = 0; d < D; ++d)
#pragma unroll
            for (int f = d + 1; f < D; ++f) {
                hu[d][f] = make_double2(row[c], row[c + 1]);
                c += 2;
            }
#pragma unroll
        for (int d = 0; d < D; ++d) b[d] = make_double2(row[D * D + 2 * d], row[D * D + 2 * d + 1]);
#pragma unroll
        for (int a = 0; a < NS; ++a) row[a] = 0.0;
#pragma unroll
        for (int d = 0; d < D; ++d) go[d] = g[(int64_t)d * cells + e];
        bool ok = true;
#pragma unroll
        for (int j = 0; j < D; ++j) {
            double v = hd[j];
#pragma unroll
            for (int k = 0; k < j; ++k) v -= norm2(L[j][k]) * dj[k];
            dj[j] = v;
            ok = ok && v > 1e-12 * hd[j];
#pragma unroll
            for (int i = j + 1; i < D; ++i) {
                double2 w = make_double2(hu[j][i].x, -hu[j][i].y);  // H[i,j] = conj(H[j,i])
#pragma unroll
                for (int k = 0; k < j; ++k) {
                    const double2 t = cmulc(L[i][k], L[j][k]);
                    w = make_double2(w.x - t.x * dj[k], w.y - t.y * dj[k]);
                }
                L[i][j] = make_double2(w.x / v, w.y / v);
            }
        }
        if (ok) {
#pragma unroll
            for (int i = 0; i < D; ++i) {  // L y = b
                double2 y = b[i];
#pragma unroll
                for (int k = 0; k < i; ++k) {
                    const double2 t = cmul(L[i][k], x[k]);
                    y = make_double2(y.x - t.x, y.y - t.y);
                }
                x[i] = y;
            }
#pragma unroll
            for (int i = 0; i < D; ++i) x[i] = make_double2(x[i].x / dj[i], x[i].y / dj[i]);
#pragma unroll
            for (int i = D - 1; i >= 0; --i) {  // L^H g' = y / d
                double2 y = x[i];
#pragma unroll
                for (int k = i + 1; k < D; ++k) {
                    const double2 t = cmulc(x[k], L[k][i]);  // conj(L[k,i]) g'[k]
                    y = make_double2(y.x - t.x, y.y - t.y);
                }
                x[i] = y;
            }
            ever[e] = 1u;
        }
#pragma unroll
        for (int d = 0; d < D; ++d) {
            double2 gn = go[d];
            if (ok) {
                gn = x[d];
                if (mode == 1) {
                    const double a = sqrt(norm2(gn));
                    gn = a > 0.0 ? make_double2(gn.x / a, gn.y / a) : go[d];
                }
                if (odd) gn = make_double2((gn.x + go[d].x) / 2.0, (gn.y + go[d].y) / 2.0);
                g[(int64_t)d * cells + e] = gn;
            }
            d2 += norm2(make_double2(gn.x - go[d].x, gn.y - go[d].y));
            s2 += norm2(gn);
        }
    }
    gc_close_iteration(d2, s2, tol, st, lds);
}

// the corrupted model of direction d at visibility k, every product rounded
__device__ __forceinline__ double2 dd_term(const double2 *__restrict__ g, const double2 *__restrict__ mod, int64_t n,
                                           int64_t cells, int d, int64_t k, int64_t ep, int64_t eq)
{
    return cmulc(cmul(g[(int64_t)d * cells + ep], mod[(int64_t)d * n + k]), g[(int64_t)d * cells + eq]);
}

// chi^2 over the used visibilities with the final gains, one partial sum per work-group
__global__ void __launch_bounds__(256)
    ddcal_chi_kernel(int64_t n, int64_t A, int64_t T, int D, const int64_t *__restrict__ a1, const int64_t *__restrict__ a2,
                     const int64_t *__restrict__ slot, const double2 *__restrict__ g, const double2 *__restrict__ vis,
                     const double2 *__restrict__ mod, const double *__restrict__ wt, double *__restrict__ parts)
{
#pragma clang fp contract(off)
    __shared__ double lds[16];
    const int64_t k0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, step = (int64_t)gridDim.x * blockDim.x;
    double chi = 0.0;
    for (int64_t k = k0; k < n; k += step) {
        int64_t p, q, t;
        double s;
        if (classify(k, A, T, a1, a2, slot, wt, &p, &q, &t, &s) != 0) continue;
        double2 r = vis[k];
        for (int d = 0; d < D; ++d) {
            const double2 m = dd_term(g, mod, n, A * T, d, k, t * A + p, t * A + q);
            r = make_double2(r.x - m.x, r.y - m.y);
        }
        chi += s * norm2(r);
    }
    chi = block_sum(chi, lds);
    if (threadIdx.x == 0) parts[blockIdx.x] = chi;
}

// vout = vin (null: zero) - the terms of the directions in dirs, ascending (vin null: + the terms).  vout may be vin
// (element k is read before it is written, by the same lane): no __restrict__ on those.
__global__ void __launch_bounds__(256)
    dd_subtract_kernel(int64_t n, int64_t A, int64_t T, int D, const int64_t *__restrict__ a1,
                       const int64_t *__restrict__ a2, const int64_t *__restrict__ slot, const double2 *__restrict__ g,
                       const double2 *__restrict__ mod, unsigned int dirs, const double2 *vin, double2 *vout)
{
#pragma clang fp contract(off)
    const int64_t k0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, step = (int64_t)gridDim.x * blockDim.x;
    for (int64_t k = k0; k < n; k += step) {
        const int64_t p = a1[k], q = a2[k], t = slot ? slot[k] : 0;
        double2 r = vin ? vin[k] : make_double2(0.0, 0.0);
        if (p >= 0 && p < A && q >= 0 && q < A && t >= 0 && t < T)
            for (int d = 0; d < D; ++d) {
                if (!(dirs >> d & 1u)) continue;
                const double2 m = dd_term(g, mod, n, A * T, d, k, t * A + p, t * A + q);
                r = vin ? make_double2(r.x - m.x, r.y - m.y) : make_double2(r.x + m.x, r.y + m.y);
            }
        vout[k] = r;
    }
}

// what gc_solve_run needs of this module: its launches; every plane of the gains [D][T][A] takes its own rotation
template <int D>
struct DdSolve : DdMod<D> {
    static constexpr int BLOCK = 0, RESIDENT = 0, RAISE_BIT = D;
    static constexpr int64_t LDS_MOST = DD_LDS_BUDGET;
    static constexpr bool PAIR = true;  // s V
    static const void *walker() { return reinterpret_cast<const void *>(ddcal_iter_kernel<D>); }
    static int64_t lds_antennas() { return gridhip_ddcal_lds_antennas(D); }
    static GcPlanes planes(const GcCall &c) { return {D, c.A * c.T, 1, true, 0u}; }
    static void init(gridhip_ctx *ctx, const GcCall &c, const GcWork &w)
    {
        hipLaunchKernelGGL(ddcal_init_kernel, grid_for(ctx, c.A * c.T * dd_sums(D)), dim3(256), 0, ctx->stream, c.A * c.T, D,
                           c.warm, w.table, w.ever, w.g);
    }
    static void prepare(gridhip_ctx *ctx, const GcCall &c, const GcWork &w)
    {
        hipLaunchKernelGGL(ddcal_prepare_kernel, w.sgrid, dim3(256), 0, ctx->stream, c.n, c.A, c.T, D, c.a1, c.a2, c.slot,
                           (const double2 *)c.vis, (const double2 *)c.model_vis, c.wt, w.pair, w.real, w.key, w.parts);
    }
    static void iter(gridhip_ctx *ctx, const GcCall &c, const GcWork &w, bool lds, dim3 grid, dim3 block, size_t bytes,
                     int64_t per)
    {
        const double2 *M = (const double2 *)c.model_vis;
        if (lds)
            hipLaunchKernelGGL(ddcal_iter_kernel<D>, grid, block, bytes, ctx->stream, c.n, (int)c.A, c.T, per,
                               (const double2 *)w.pair, (const double *)w.real, (const unsigned long long *)w.key, M,
                               (const double2 *)w.g, w.table, (const GcState *)w.st);
        else
            hipLaunchKernelGGL(ddcal_iter_global_kernel<D>, w.sgrid, dim3(256), 0, ctx->stream, c.n, c.A, c.T,
                               (const double2 *)w.pair, (const double *)w.real, (const unsigned long long *)w.key, M,
                               (const double2 *)w.g, w.table, (const GcState *)w.st);
    }
    static void update(gridhip_ctx *ctx, const GcCall &c, const GcWork &w)
    {
        hipLaunchKernelGGL(ddcal_solve_kernel<D>, dim3(1), dim3(512), 0, ctx->stream, c.A * c.T, c.mode, c.tol, w.table,
                           w.ever, w.g, w.st);
    }
    static void final(gridhip_ctx *ctx, const GcCall &c, const GcWork &w)
    {
        hipLaunchKernelGGL(ddcal_chi_kernel, w.sgrid, dim3(256), 0, ctx->stream, c.n, c.A, c.T, D, c.a1, c.a2, c.slot,
                           (const double2 *)w.g, (const double2 *)c.vis, (const double2 *)c.model_vis, c.wt, w.parts);
    }
};

// what gc_solve_any needs: the rules, and the driver of the call's D
struct DdAny {
    static GcRules rules(const GcCall &c) { return {"ddcal", 1, true, 16, 16 * (size_t)c.D, (size_t)c.D * c.A * c.T * 16}; }
    static int run(gridhip_ctx *ctx, const GcCall &c)
    {
#define DD_CASE(d) \
    case d:        \
        return gc_solve_run<DdSolve<d>>(ctx, c);
        switch (c.D) {
            DD_CASE(1) DD_CASE(2) DD_CASE(3) DD_CASE(4) DD_CASE(5) DD_CASE(6) DD_CASE(7) DD_CASE(8)
        }
#undef DD_CASE
        return GRIDHIP_EINVAL;  // (ddcal_check lets no other D through)
    }
};

}  // namespace

int ddcal_check(gridhip_ctx *ctx, int64_t n, int64_t A, int64_t T, int64_t D, const int64_t *a1, const int64_t *a2,
                const int64_t *slot, const double *vis, const double *model_vis, const double *wt, int mode, int64_t refant,
                int64_t niter, double tol, const double *gains)
{
    const GcCall c = {n, A, T, D, a1, a2, slot, vis, model_vis, wt, mode, refant, 0, niter, tol, const_cast<double *>(gains)};
    return gc_solve_check(ctx, DdAny::rules(c), c);
}

int dd_subtract_check(gridhip_ctx *ctx, int64_t n, int64_t A, int64_t T, int64_t D, const int64_t *a1, const int64_t *a2,
                      const int64_t *slot, const double *gains, const double *model_vis, int64_t dirs, const double *vis_in,
                      const double *vis_out)
{
    if (n < 0 || A < 2 || T < 1 || D < 1 || D > DD_MAX_D || (!slot && T != 1) ||
        (n > 0 && (!a1 || !a2 || !model_vis || !vis_out)) || !gains || dirs < 0 || (dirs >> D) != 0)
        return fail(ctx, GRIDHIP_EINVAL, "dd_subtract: bad argument");
    GH_CHECK(shape_check(ctx, "dd_subtract", n, A, T, a1, a2, slot, &D));
    const size_t gb = (size_t)D * A * T * 16, n8 = (size_t)n * 8;
    if (overlaps_any({vis_out, 2 * n8}, {{gains, gb}, {a1, n8}, {a2, n8}, {slot, n8}, {model_vis, 2 * n8 * D}}))
        return fail(ctx, GRIDHIP_EINVAL, "dd_subtract: vis_out overlaps gains, model_vis, a1, a2 or slot");
    if (vis_out != vis_in && overlap(vis_out, 2 * n8, vis_in, 2 * n8))
        return fail(ctx, GRIDHIP_EINVAL, "dd_subtract: vis_out may be vis_in itself, and overlap it in no other way");
    return GRIDHIP_OK;
}

int peel_check(gridhip_ctx *ctx, int64_t n, int64_t cells, const double *model_vis, const double *gains, const int64_t *a1,
               const int64_t *a2, const int64_t *slot, const double *vis, const double *wt, const double *wt_cal,
               const double *stats)
{
    const size_t n8 = (size_t)n * 8;
    if (overlap(wt_cal, n8, gains, (size_t)cells * 16))
        return fail(ctx, GRIDHIP_EINVAL, "peel: wt_cal overlaps gains");
    if (overlaps_any({model_vis, 2 * n8}, {{a1, n8}, {a2, n8}, {slot, n8}, {vis, 2 * n8}, {wt, n8}, {wt_cal, n8}, {stats, 64}}))
        return fail(ctx, GRIDHIP_EINVAL, "peel: row 0 of model_vis is written and may overlap nothing else");
    return GRIDHIP_OK;
}

int dd_subtract_run(gridhip_ctx *ctx, int64_t n, int64_t A, int64_t T, int64_t D, const int64_t *a1, const int64_t *a2,
                    const int64_t *slot, const double *gains, const double *model_vis, int64_t dirs, const double *vis_in,
                    double *vis_out)
{
    if (n == 0) return GRIDHIP_OK;
    hipLaunchKernelGGL(dd_subtract_kernel, grid_for(ctx, n), dim3(256), 0, ctx->stream, n, A, T, (int)D, a1, a2, slot,
                       (const double2 *)gains, (const double2 *)model_vis, (unsigned int)dirs, (const double2 *)vis_in,
                       (double2 *)vis_out);
    GH_CHECK_HIP(ctx, hipGetLastError());
    return GRIDHIP_OK;
}

int ddcal_run(gridhip_ctx *ctx, int64_t n, int64_t A, int64_t T, int64_t D, const int64_t *a1, const int64_t *a2,
              const int64_t *slot, const double *vis, const double *model_vis, const double *wt, int mode, int64_t refant,
              int warm, int64_t niter, double tol, double *gains, double *stats)
{
    return DdAny::run(ctx, {n, A, T, D, a1, a2, slot, vis, model_vis, wt, mode, refant, warm, niter, tol, gains, stats});
}

}  // namespace gridhip

using namespace gridhip;

namespace {

int dd_subtract_any(gridhip_ctx *ctx, bool dev, int64_t n, int64_t A, int64_t T, int64_t D, const int64_t *a1,
                    const int64_t *a2, const int64_t *slot, const double *gains, const double *model_vis, int64_t dirs,
                    const double *vis_in, double *vis_out)
{
    if (!ctx) return GRIDHIP_EINVAL;
    GH_CHECK(dd_subtract_check(ctx, n, A, T, D, a1, a2, slot, gains, model_vis, dirs, vis_in, vis_out));
    GH_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n8 = (size_t)n * 8;
    Staged st(ctx, dev);
    a1 = st.in(a1, n8), a2 = st.in(a2, n8), slot = st.in(slot, n8), gains = st.in(gains, (size_t)D * A * T * 16);
    model_vis = st.in(model_vis, 2 * n8 * D), vis_out = st.inout(vis_in, vis_out, 2 * n8);
    if (!dev && vis_in) vis_in = vis_out;  // (the staged visibilities are subtracted from in place)
    GH_CHECK(st.status());
    GH_CHECK(dd_subtract_run(ctx, n, A, T, D, a1, a2, slot, gains, model_vis, dirs, vis_in, vis_out));
    return st.finish();
}

}  // namespace

extern "C" {

int64_t gridhip_ddcal_lds_antennas(int64_t D)
{
    return D < 1 || D > DD_MAX_D ? 0 : DD_LDS_BUDGET / ((D * D + 4 * D) * 8);
}

int gridhip_ddcal_dev(gridhip_ctx *ctx, int64_t n, int64_t A, int64_t T, int64_t D, const int64_t *a1, const int64_t *a2,
                      const int64_t *slot, const double *vis, const double *model_vis, const double *wt, int mode,
                      int64_t refant, int warm, int64_t niter, double tol, double *gains, double *stats)
{
    return gc_solve_any<DdAny>(ctx, true, {n, A, T, D, a1, a2, slot, vis, model_vis, wt, mode, refant, warm, niter, tol,
                                           gains, stats});
}

int gridhip_ddcal(gridhip_ctx *ctx, int64_t n, int64_t A, int64_t T, int64_t D, const int64_t *a1, const int64_t *a2,
                  const int64_t *slot, const double *vis, const double *model_vis, const double *wt, int mode,
                  int64_t refant, int warm, int64_t niter, double tol, double *gains, double *stats)
{
    return gc_solve_any<DdAny>(ctx, false, {n, A, T, D, a1, a2, slot, vis, model_vis, wt, mode, refant, warm, niter, tol,
                                            gains, stats});
}

int gridhip_dd_subtract_dev(gridhip_ctx *ctx, int64_t n, int64_t A, int64_t T, int64_t D, const int64_t *a1,
                            const int64_t *a2, const int64_t *slot, const double *gains, const double *model_vis,
                            int64_t dirs, const double *vis_in, double *vis_out)
{
    return dd_subtract_any(ctx, true, n, A, T, D, a1, a2, slot, gains, model_vis, dirs, vis_in, vis_out);
}

int gridhip_dd_subtract(gridhip_ctx *ctx, int64_t n, int64_t A, int64_t T, int64_t D, const int64_t *a1, const int64_t *a2,
                        const int64_t *slot, const double *gains, const double *model_vis, int64_t dirs,
                        const double *vis_in, double *vis_out)
{
    return dd_subtract_any(ctx, false, n, A, T, D, a1, a2, slot, gains, model_vis, dirs, vis_in, vis_out);
}

}  // extern "C"
