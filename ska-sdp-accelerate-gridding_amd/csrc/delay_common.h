// What the delay-like calibrations (fringe.hip: delay and rate; tec.hip: delay and TEC) share beyond delay_arith.h: the
// bookkeeping of a search, the fields of a search every module stages alike, the sample before its derotation, the
// work-group's reduction to one candidate, the ends of the refinement, the apply step, the host rules and the fit driver.
// CONTRACTION IS OFF FROM HERE ON, by the pragma below the includes, which belongs to this header as it does to
// delay_arith.h (which says why): the build passes no -ffp-contract flag, and a fused product changes pinned bits.
//
// A module hands the templates below a struct M of static members (FrMod, TcMod): its search struct and table head
// (Search on DlSearch; Head with ok, I, tint, made by head()), the rotation of a sample under two antennas' solutions
// (rotate), whether a table fits a driver's call and the steps of its axes (fit_steps), its limits and names for
// messages, its table sizes, the cells and tile counts of a driver's round (round, tiles, groups) and its search_launch.
#pragma once
#include "delay_arith.h"
#include "fringe_solve.h"
#include "imaging.h"

#pragma clang fp contract(off)

namespace gridhip {

namespace {

// ---- a search: its counters, its fields, its sample, its candidates -----------------------------------------------------

struct DlCount {  // the counters of one search
    u64 flagged, bad, empty, refused, ok;
    u64 pad[3];
};

// what every search struct starts with; a module adds its window and its tile counts
struct DlSearch {
    int B, T, F, A;
    const double *tables;
    const double2 *vis, *model;
    const double *wt;
    const int64_t *a1, *a2;
    const double *sol;
    int mode;      // 0: the cells the call names; 1: those within the call's half-widths of the grid's zero; 2: the whole grid
    int Ib;        // the caller's I: the table's, or the call does not fit
    double *cand;  // [B][Ib][tiles][4] = { P, j, k, 0 }, P = -1: none
    double *peaks;
    DlCount *cnt;
};

__global__ void dl_zero_kernel(DlCount *cnt)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) *cnt = DlCount{};
}

// S: a module's search struct; S::fits(): its head and its window take the call
template <class S>
__global__ void dl_search_stats_kernel(S a, double *__restrict__ stats)
{
    if (blockIdx.x != 0 || threadIdx.x != 0 || !stats) return;
    const bool ok = a.fits();
    for (int i = 0; i < DL_STATS; ++i) stats[i] = 0.0;
    if (ok) {
        stats[0] = (double)a.cnt->flagged, stats[1] = (double)a.cnt->bad, stats[2] = (double)a.cnt->empty;
        stats[3] = (double)a.cnt->refused, stats[4] = (double)a.cnt->ok;
    } else {
        stats[7] = 1.0;
    }
}

// X' of the sample at `at`: the weight times the visibility times the conjugate model, then the module's derotation of
// that (its products differ in number and order, so they stay the module's); *flagged: its weight is not > 0 and it is
// (0, 0), underotated
template <class D>
__device__ __forceinline__ double2 dl_sample(const DlSearch &a, int64_t at, bool *flagged, D derotate)
{
    const double s = a.wt ? a.wt[at] : 1.0;
    *flagged = !(s > 0.0);
    if (*flagged) return make_double2(0.0, 0.0);
    const double2 v = a.vis[at];
    double2 x = make_double2(s * v.x, s * v.y);
    if (a.model) x = dl_mulc(x, a.model[at]);
    return derotate(x);
}

__device__ __forceinline__ void dl_put_cand(double *c, double p, int j, int k) { c[0] = p, c[1] = (double)j, c[2] = (double)k, c[3] = 0.0; }

// the best of the lanes' (P, j, k) of a work-group of W waves by dl_ahead, in thread 0 alone; tid: threadIdx.x; rp, rj,
// rk: a slot per wave in LDS, with a barrier of the caller's between two uses
template <int W>
__device__ __forceinline__ void dl_group_best(int tid, double &bp, int &bj, int &bk, double *rp, int *rj, int *rk)
{
    for (int o = 32; o > 0; o >>= 1) {
        const double qp = __shfl_xor(bp, o);
        const int qj = __shfl_xor(bj, o), qk = __shfl_xor(bk, o);
        if (dl_ahead(qp, qj, qk, bp, bj, bk)) bp = qp, bj = qj, bk = qk;
    }
    if ((tid & 63) == 0) rp[tid >> 6] = bp, rj[tid >> 6] = bj, rk[tid >> 6] = bk;
    __syncthreads();
    if (tid == 0)
        for (int w = 1; w < W; ++w)
            if (dl_ahead(rp[w], rj[w], rk[w], bp, bj, bk)) bp = rp[w], bj = rj[w], bk = rk[w];
}

// ---- the ends of a refinement -------------------------------------------------------------------------------------------

// the best candidate of a (baseline, interval) over the u1 x u2 tiles its window uses, of rows of n2 tiles at cb.  The
// rule is dl_ahead's, whatever the order of the tiles.  A tile without a candidate holds (-1, -1, -1), which is ahead of
// nothing - the start value included - so no test of P >= 0 is needed.  Where the tiles divide the first axis alone and
// ascend with it (fringe: u2 = n2 = 1), equal powers of a later tile have a higher first index and lose, so this is the
// first tile of the strictly largest power.
__device__ __forceinline__ void dl_best_tile(const double *cb, int u1, int u2, int n2, double *bp, int *bj, int *bk)
{
    *bp = -1.0, *bj = -1, *bk = -1;
    for (int t1 = 0; t1 < u1; ++t1)
        for (int t2 = 0; t2 < u2; ++t2) {
            const double *c = cb + ((int64_t)t1 * n2 + t2) * 4;
            if (dl_ahead(c[0], (int)c[1], (int)c[2], *bp, *bj, *bk)) *bp = c[0], *bj = (int)c[1], *bk = (int)c[2];
        }
}

// a row without a peak, but for its count [8] and its class [10]
__device__ __forceinline__ void dl_row_none(double *out)
{
    out[0] = -1.0, out[1] = -1.0, out[2] = 0.0, out[3] = 0.0, out[4] = 0.0, out[5] = 1.0, out[6] = 0.0, out[7] = 0.0;
    out[9] = 0.0;
}

// the row of the peak (bj, bk), for a whole wave: lane 0 holds S there, lanes 1 and 2 at bj -+ 1 (in1: they exist),
// lanes 3 and 4 at bk -+ 1 (in2).  N: the energy of the nu used samples; (o1, d1), (o2, d2): the origin and the step of
// either axis.  False: the power at the peak is a NaN.
__device__ __forceinline__ bool dl_peak_row(double *out, int bj, int bk, bool in1, bool in2, double2 S, double N, int nu, double o1,
                                            double d1, double o2, double d2)
{
    const double P = S.x * S.x + S.y * S.y;
    const double ps = __shfl(P, 0), p1m = __shfl(P, 1), p1p = __shfl(P, 2), p2m = __shfl(P, 3), p2p = __shfl(P, 4);
    const double sre = __shfl(S.x, 0), sim = __shfl(S.y, 0);
    double x1 = o1 + (double)bj * d1, x2 = o2 + (double)bk * d2;
    if (in1) x1 = x1 + dl_parabola(p1m, ps, p1p) * d1;
    if (in2) x2 = x2 + dl_parabola(p2m, ps, p2p) * d2;
    out[0] = (double)bj, out[1] = (double)bk, out[2] = ps, out[3] = x1, out[4] = x2;
    if (ps > 0.0) {
        const double sq = sqrt(ps);
        out[5] = sre / sq, out[6] = sim / sq;
    }
    out[7] = N > 0.0 ? ps / ((double)nu * N) : 0.0;
    out[9] = N;
    return ps == ps;
}

// one thread writes the row of class `code` - one that failed holds no peak - and counts it
__device__ __forceinline__ void dl_put_row(DlCount *cnt, double *row, double *out, int code, u64 nflag)
{
    if (code != 0) dl_row_none(out);
    out[10] = (double)code;
#pragma unroll
    for (int c = 0; c < DL_ROW; ++c) row[c] = out[c];
    if (nflag) atomicAdd(&cnt->flagged, nflag);
    atomicAdd(code == 0 ? &cnt->ok : code == 1 ? &cnt->empty : code == 2 ? &cnt->bad : &cnt->refused, (u64)1);
}

// ---- the apply step -----------------------------------------------------------------------------------------------------

struct DlApply {
    int B, T, F, A, I;
    const double *tables, *sol;
    const int64_t *a1, *a2;
    int inverse;
    const double2 *vis_in;
    const double *wt_in;
    double2 *vis_out;
    double *wt_out;
};

template <class M>
__global__ void __launch_bounds__(256) dl_apply_kernel(DlApply a)
{
    const typename M::Head h = M::head(a.tables, a.T, a.F);
    if (!h.ok || h.I != a.I) return;
    const int64_t n = (int64_t)a.B * a.T * a.F;
    const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, step = (int64_t)gridDim.x * blockDim.x;
    for (int64_t at = i0; at < n; at += step) {
        const int f = (int)(at % a.F);
        const int64_t bt = at / a.F;
        const int t = (int)(bt % a.T), b = (int)(bt / a.T), i = t / h.tint;
        const int64_t p = a.a1[b], q = a.a2[b];
        double2 v = a.vis_in[at];
        const double wv = a.wt_in ? a.wt_in[at] : 1.0;
        bool ok = p >= 0 && p < a.A && q >= 0 && q < a.A;
        if (ok) {
            const double *sp = a.sol + ((int64_t)i * a.A + p) * 4, *sq = a.sol + ((int64_t)i * a.A + q) * 4;
            ok = dl_finite(sp[0]) && dl_finite(sp[1]) && dl_finite(sp[2]) && dl_finite(sp[3]) && dl_finite(sq[0]) &&
                 dl_finite(sq[1]) && dl_finite(sq[2]) && dl_finite(sq[3]);
            if (ok) v = M::rotate(h, f, t, sp, sq, a.inverse, v);
        }
        a.vis_out[at] = v;
        if (a.wt_out) a.wt_out[at] = ok ? wv : 0.0;
    }
}

// ---- the host rules -----------------------------------------------------------------------------------------------------

// does the head of a host form's table, in host memory, fit the cube?  Then the call stages the whole table, else the
// head alone (the kernels see the same head and leave).  n1, n2: the cells of its axes, within max_n1, max_n2
inline bool dl_host_head_fits(const double *tables, int64_t T, int64_t F, int64_t max_tint, int64_t max_n1, int64_t max_n2)
{
    const double tint = tables[3], n1 = tables[5], n2 = tables[6];
    return tables[0] == 1.0 && tables[1] == (double)F && tables[2] == (double)T && tint >= 1.0 && tint <= (double)max_tint &&
           tint == (double)(int64_t)tint && n1 >= 1.0 && n1 <= (double)max_n1 && n1 == (double)(int64_t)n1 && n2 >= 1.0 &&
           n2 <= (double)max_n2 && n2 == (double)(int64_t)n2;
}

// the fields of DlSearch but sol and mode, which are the call's: the cube, the staged table and arrays, the scratch
inline void dl_stage_search(Staged &sg, DlSearch &a, int64_t B, int64_t T, int64_t F, int64_t A, int64_t I, const double *tables,
                            size_t tb, const double *vis, const double *model_vis, const double *wt, const int64_t *a1,
                            const int64_t *a2, double *peaks, DevBuf &cand, DevBuf &cnt)
{
    const size_t n = (size_t)B * T * F, ib = (size_t)B * 8;
    a.B = (int)B, a.T = (int)T, a.F = (int)F, a.A = (int)A;
    a.tables = sg.in(tables, tb);
    a.vis = reinterpret_cast<const double2 *>(sg.in(vis, n * 16));
    a.model = reinterpret_cast<const double2 *>(sg.in(model_vis, n * 16));
    a.wt = sg.in(wt, n * 8), a.a1 = sg.in(a1, ib), a.a2 = sg.in(a2, ib);
    // (a table that does not fit leaves the peaks as they are, in the host form too)
    a.peaks = sg.inout(peaks, peaks, (size_t)B * I * DL_ROW * 8);
    a.Ib = (int)I, a.cand = cand.as<double>(), a.cnt = cnt.as<DlCount>();
}

template <class M>
int dl_apply_any(gridhip_ctx *ctx, bool dev, int64_t B, int64_t T, int64_t F, int64_t A, int64_t I, const double *tables,
                 const double *sol, const int64_t *a1, const int64_t *a2, int inverse, const double *vis_in,
                 const double *wt_in, double *vis_out, double *wt_out)
{
    if (!ctx) return GRIDHIP_EINVAL;
    if (!dl_cube_ok(B, T, F, A, M::MAX_F) || I < 1 || I > T || !tables || !sol || !a1 || !a2 || !vis_in || !vis_out ||
        (inverse != 0 && inverse != 1) || ((uintptr_t)vis_in & 15) || ((uintptr_t)vis_out & 15))
        return fail(ctx, GRIDHIP_EINVAL, "%s: bad argument", M::apply_name);
    if (!dl_cube_fits(B, T, A)) return fail(ctx, GRIDHIP_EUNSUPPORTED, "%s: B above 2^24, T above 2^20 or A above 1024", M::apply_name);
    const size_t tb = dev ? (size_t)DL_HEAD * 8 : M::host_table_bytes(tables, T, F);
    const size_t n = (size_t)B * T * F, sb = (size_t)I * A * 32, ib = (size_t)B * 8;
    if (outputs_clash({{vis_out, n * 16}, {wt_out, n * 8}},
                      {{vis_in, n * 16}, {wt_in, n * 8}, {tables, tb}, {sol, sb}, {a1, ib}, {a2, ib}}, {{0, 0}, {1, 1}}))
        return fail(ctx, GRIDHIP_EINVAL, "%s: arrays overlap", M::apply_name);
    GH_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    Staged sg(ctx, dev);
    DlApply a{};
    a.B = (int)B, a.T = (int)T, a.F = (int)F, a.A = (int)A, a.I = (int)I, a.inverse = inverse;
    a.tables = sg.in(tables, tb), a.sol = sg.in(sol, sb), a.a1 = sg.in(a1, ib), a.a2 = sg.in(a2, ib);
    // a table that does not fit leaves the outputs as they are, in the host form too: an output's block starts from the
    // output's own bytes, and is the input's block only in place
    a.vis_out = reinterpret_cast<double2 *>(sg.inout(vis_out, vis_out, n * 16));
    a.vis_in = vis_in == vis_out ? a.vis_out : reinterpret_cast<const double2 *>(sg.in(vis_in, n * 16));
    a.wt_out = sg.inout(wt_out, wt_out, n * 8);
    a.wt_in = !wt_out ? nullptr : wt_in == wt_out ? a.wt_out : sg.in(wt_in, n * 8);  // (read only for wt_out)
    GH_CHECK(sg.status());
    hipLaunchKernelGGL(dl_apply_kernel<M>, grid_for(ctx, (int64_t)n), dim3(256), 0, ctx->stream, a);
    GH_CHECK_HIP(ctx, hipGetLastError());
    return sg.finish();
}

// ---- the fit driver -----------------------------------------------------------------------------------------------------

// the driver's stats from those of its last search (ss) and solve (vs)
template <class M>
__global__ void dl_fit_stats_kernel(int T, int F, int I, int N1, int N2, const double *__restrict__ tables,
                                    const double *__restrict__ ss, const double *__restrict__ vs, double *__restrict__ stats)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    double d1, d2;
    const bool ok = M::fit_steps(tables, T, F, I, N1, N2, &d1, &d2);
    for (int i = 0; i < DL_STATS; ++i) stats[i] = 0.0;
    if (!ok || ss[7] != 0.0) {
        stats[7] = 1.0;
        return;
    }
    stats[0] = vs[0], stats[1] = ss[0], stats[2] = ss[1], stats[3] = ss[2], stats[4] = vs[2];
    stats[5] = vs[4] / d1, stats[6] = vs[5] / d2;
}

// rounds of a search and the antenna fit of fringe_solve.hip: the whole grid first (derotated only on a warm start), then
// windows of (w1, w2) cells about the grid's zero under the solution so far
template <class M>
int dl_fit_any(gridhip_ctx *ctx, bool dev, int64_t B, int64_t T, int64_t F, int64_t A, int64_t I, int64_t N1, int64_t N2,
               const double *tables, const double *vis, const double *model_vis, const double *wt, const int64_t *a1,
               const int64_t *a2, int64_t rounds, int64_t w1, int64_t w2, double min_count, double min_coh2, int64_t refant,
               int64_t niter, double tol, int warm, double *sol, double *peaks, double *info, double *stats)
{
    if (!ctx) return GRIDHIP_EINVAL;
    if (!dl_cube_ok(B, T, F, A, M::MAX_F) || I < 1 || I > T || N1 < 1 || N1 > M::MAX_N1 || N2 < 1 || N2 > M::MAX_N2 || !tables ||
        !vis || !a1 || !a2 || !sol || !peaks || !info || !stats || rounds < 1 || rounds > M::MAX_ROUNDS || w1 < 0 ||
        w1 > M::MAX_N1 || w2 < 0 || w2 > M::MAX_N2 || (warm != 0 && warm != 1) ||
        !fr_solve_args_ok(B, I, A, min_count, min_coh2, refant, niter, tol) || ((uintptr_t)vis & 15) ||
        ((uintptr_t)model_vis & 15))
        return fail(ctx, GRIDHIP_EINVAL, "%s: bad argument", M::fit_name);
    typename M::Search a{};
    M::round(a, true, N1, N2, w1, w2);
    const int64_t nt0 = M::tiles(a), g0 = M::groups(a, B, I);
    M::round(a, false, N1, N2, w1, w2);
    const int64_t nt1 = M::tiles(a), g1 = M::groups(a, B, I), ntmax = nt0 > nt1 ? nt0 : nt1;
    if (!dl_cube_fits(B, T, A) || B * T > ((int64_t)1 << 31) - 1 || (g0 > g1 ? g0 : g1) > 0x7fffffffLL)
        return fail(ctx, GRIDHIP_EUNSUPPORTED, "%s: B above 2^24, T above 2^20, A above 1024, or too many tiles", M::fit_name);
    const size_t n = (size_t)B * T * F, tb = M::table_bytes(F, T, N1, N2), pb = (size_t)B * I * DL_ROW * 8;
    const size_t sb = (size_t)I * A * 32, nb = (size_t)I * A * 8, ib = (size_t)B * 8;
    if (outputs_clash({{sol, sb}, {peaks, pb}, {info, nb}, {stats, 64}},
                      {{tables, tb}, {vis, n * 16}, {model_vis, n * 16}, {wt, n * 8}, {a1, ib}, {a2, ib}}))
        return fail(ctx, GRIDHIP_EINVAL, "%s: arrays overlap", M::fit_name);
    GH_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    DevBuf cnt, cand, w, part, st, edges;
    GH_CHECK(cnt.alloc(ctx, sizeof(DlCount)));
    GH_CHECK(cand.alloc(ctx, (size_t)B * I * ntmax * 32));
    GH_CHECK(w.alloc(ctx, (size_t)I * B * 8));
    GH_CHECK(part.alloc(ctx, (size_t)I * 64));
    GH_CHECK(st.alloc(ctx, 128));
    GH_CHECK(edges.alloc(ctx, (size_t)I * B * 2 * sizeof(FrEdge)));
    Staged sg(ctx, dev);
    dl_stage_search(sg, a, B, T, F, A, I, tables, tb, vis, model_vis, wt, a1, a2, peaks, cand, cnt);
    double *dsol = sg.inout(sol, sol, sb);
    double *dinfo = sg.inout(info, info, nb);
    stats = sg.out(stats, 64);
    GH_CHECK(sg.status());
    FrSolve v{};
    v.B = (int)B, v.I = (int)I, v.A = (int)A, v.a1 = a.a1, v.a2 = a.a2, v.peaks = a.peaks;
    v.min_count = min_count, v.min_coh2 = min_coh2, v.refant = (int)(refant < 0 ? -1 : refant), v.niter = (int)niter, v.tol = tol;
    v.sol = dsol, v.info = dinfo, v.w = w.as<double>(), v.part = part.as<double>(), v.edges = edges.as<FrEdge>();
    double *ss = st.as<double>(), *vs = ss + 8;
    v.gate = ss;
    if (!warm) fr_init_sol_launch(ctx, I * A, dsol);
    for (int64_t r = 0; r < rounds; ++r) {
        M::round(a, r == 0, N1, N2, w1, w2);
        a.sol = r == 0 && !warm ? nullptr : dsol;
        M::search_launch(ctx, a, I, ss);
        fr_solve_launch(ctx, v, vs);
    }
    hipLaunchKernelGGL(dl_fit_stats_kernel<M>, dim3(1), dim3(64), 0, ctx->stream, (int)T, (int)F, (int)I, (int)N1, (int)N2, a.tables,
                       (const double *)ss, (const double *)vs, stats);
    GH_CHECK_HIP(ctx, hipGetLastError());
    return sg.finish();
}

}  // namespace

}  // namespace gridhip
