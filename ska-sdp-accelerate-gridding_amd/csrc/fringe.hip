// Delay and rate calibration (include/gridhip.h, "delay and rate calibration"): a fringe search per baseline and solution
// interval over a grid of delays and rates, an antenna-based fit of the baseline values, and the apply step.
//
//     gridhip_fringe_tables   fr_head_kernel (one thread: the checks, the head), fr_fill_kernel (one thread per entry)
//     gridhip_fringe_search   dl_zero_kernel, fr_search_kernel, fr_refine_kernel, dl_search_stats_kernel<FrSearch>
//     gridhip_fringefit       dl_fit_any<FrMod>: [the solve's init]; per round the four above and the two of the solve;
//                             dl_fit_stats_kernel<FrMod>
//     gridhip_apply_fringe    dl_apply_kernel<FrMod> (one thread per sample)
// The dl_ names are delay_common.h's, which tec.hip uses alike: the rounded arithmetic, the counters, the sample before
// its derotation, the reduction to a candidate, the ends of the refinement, the apply step, the host rules and the fit
// driver.  This file owns the table, the window, the derotation and the two large kernels, and FrMod, which tells the
// shared templates about them.  The antenna fit (gridhip_fringe_solve) is fringe_solve.hip.
// Every kernel that reads a table judges its head itself and leaves at once when it does not fit the call; nothing is
// read back, so every _dev form is a fixed chain of launches.
//
// THE SEARCH KERNEL.  A work-group of 256 threads owns one baseline and FR_TJ = 8 delays and walks the solution
// intervals; per interval it forms S[j][k] = sum_t Et[t][k] (sum_f Ef[f][j] X'[t][f]) in two ordered sums:
//   1. lane (ty, tx) = (tid / 8, tid % 8) keeps Y[t][j] of the delay tx and the time steps ty, ty + 32, ... (at most 8
//      complex accumulators, tint <= 256) in registers.  X' - weighted, multiplied by the conjugate model, derotated by
//      the current solution - and Ef stream through LDS in chunks of FR_KC = 8 channels (32 KB at tint = 256); every
//      accumulator adds its channels in ascending order, unfused.  The derotation phasors of the (baseline, interval)
//      are made once into LDS (20 KB).
//   2. Y is parked in LDS over the staging buffer; lane (ty, tx) then forms S of the delay tx and the rates k0 + ty,
//      k0 + ty + 32, ... against Et read from global memory, t ascending, and keeps a running (P, j, k) maximum, which
//      is reduced over the work-group by the tie rule (largest P, lowest j, lowest k) into one candidate per tile.
// 53 KB of LDS per work-group: two share a CU.  No matrix instruction (v_mfma_f64 fixes its own order and fuses).
// THE REFINEMENT KERNEL.  One wave per (baseline, interval) takes the best candidate over the tiles in ascending order,
// recomputes S at the peak and its four neighbours by the same two ordered sums from the same device functions - so the
// bits do not depend on the tile borders - and forms the energy, the counts and the row of `peaks`.
#include "delay_common.h"

#pragma clang fp contract(off)

namespace gridhip {

namespace {

constexpr int FR_THREADS = 256;
constexpr int FR_TJ = 8;                     // delays of a work-group
constexpr int FR_KC = 8;                     // channels of a staged chunk
constexpr int FR_TR = FR_THREADS / FR_TJ;    // rates of a lane-pass, and the time steps of a pass of the first sum
constexpr int FR_HEAD = DL_HEAD, FR_ROW = DL_ROW;
constexpr int FR_MAX_F = GRIDHIP_FRINGE_MAX_CHANNELS, FR_MAX_ND = GRIDHIP_FRINGE_MAX_DELAYS;
constexpr int FR_MAX_TINT = GRIDHIP_FRINGE_MAX_TINT, FR_MAX_NR = GRIDHIP_FRINGE_MAX_RATES;
constexpr int FR_NT = FR_MAX_TINT / FR_TR;   // accumulators of a lane in the first sum
static_assert(FR_TJ * FR_KC <= FR_THREADS && FR_NT * FR_TR == FR_MAX_TINT, "the search kernel's staging");

struct FrHead {
    bool ok;
    int F, T, tint, I, Nd, Nr;
    double tau0, dtau, r0, drate;
    const double2 *Ef, *Et;
    const double *tref, *af, *dtm;
};

// the head of a table, and whether it fits a cube of T time steps and F channels
__device__ __forceinline__ FrHead fr_head(const double *tb, int T, int F)
{
    FrHead h;
    h.ok = tb[0] == 1.0 && tb[1] == (double)F && tb[2] == (double)T && dl_int_in(tb[3], 1, FR_MAX_TINT) &&
           dl_int_in(tb[5], 1, FR_MAX_ND) && dl_int_in(tb[6], 1, FR_MAX_NR) && F >= 1 && F <= FR_MAX_F && T >= 1;
    h.F = F, h.T = T;
    h.tint = h.ok ? (int)tb[3] : 1, h.Nd = h.ok ? (int)tb[5] : 1, h.Nr = h.ok ? (int)tb[6] : 1;
    h.I = (T + h.tint - 1) / h.tint;
    h.ok = h.ok && tb[4] == (double)h.I;
    h.tau0 = tb[7], h.dtau = tb[8], h.r0 = tb[9], h.drate = tb[10];
    const double *p = tb + FR_HEAD;
    h.Ef = reinterpret_cast<const double2 *>(p), p += 2 * (int64_t)F * h.Nd;
    h.Et = reinterpret_cast<const double2 *>(p), p += 2 * (int64_t)T * h.Nr;
    h.tref = p, h.af = p + T, h.dtm = h.af + F;
    return h;
}

__global__ void __launch_bounds__(256)
    fr_head_kernel(int F, int T, int tint, int Nd, int Nr, const double *__restrict__ freq, const double *__restrict__ time,
                   double tau0, double dtau, double r0, double drate, double *__restrict__ tables)
{
    if (blockIdx.x != 0) return;
    int bad = 0;  // the one work-group shares the scan of freq and time
    for (int i = threadIdx.x; i < F + T; i += blockDim.x) bad |= !dl_finite(i < F ? freq[i] : time[i - F]);
    bad = __syncthreads_or(bad);
    if (threadIdx.x != 0) return;
    const double nu0 = freq[0] + 0.5 * (freq[F - 1] - freq[0]);
    const bool ok = !bad && dl_finite(tau0) && dl_finite(dtau) && dl_finite(r0) && dl_finite(drate) && dtau > 0.0 &&
                    drate > 0.0 && dl_finite(nu0);
    for (int i = 0; i < FR_HEAD; ++i) tables[i] = 0.0;
    tables[0] = ok ? 1.0 : 0.0;
    tables[1] = (double)F, tables[2] = (double)T, tables[3] = (double)tint, tables[4] = (double)((T + tint - 1) / tint);
    tables[5] = (double)Nd, tables[6] = (double)Nr, tables[7] = tau0, tables[8] = dtau, tables[9] = r0, tables[10] = drate;
    tables[11] = ok ? nu0 : 0.0;
}

__global__ void __launch_bounds__(256)
    fr_fill_kernel(int F, int T, int tint, int Nd, int Nr, const double *__restrict__ freq, const double *__restrict__ time,
                   double *tables)
{
    const bool valid = tables[0] == 1.0;
    const double tau0 = tables[7], dtau = tables[8], r0 = tables[9], drate = tables[10], nu0 = tables[11];
    const int I = (T + tint - 1) / tint;
    const int64_t nF = (int64_t)F * Nd, nT = (int64_t)T * Nr, total = nF + nT + 2 * (int64_t)T + F;
    double *Ef = tables + FR_HEAD, *Et = Ef + 2 * nF, *tref = Et + 2 * nT, *af = tref + T, *dtm = af + F;
    const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, step = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = i0; i < total; i += step) {
        if (i < nF) {
            double2 e = make_double2(0.0, 0.0);
            if (valid) {
                const int f = (int)(i / Nd), j = (int)(i % Nd);
                e = dl_phasor(tau0 + (double)j * dtau, freq[f] - nu0);
            }
            Ef[2 * i] = e.x, Ef[2 * i + 1] = -e.y;
        } else if (i < nF + nT) {
            const int64_t m = i - nF;
            double2 e = make_double2(0.0, 0.0);
            if (valid) {
                const int t = (int)(m / Nr), k = (int)(m % Nr);
                const int ta = (t / tint) * tint, tb = ta + tint < T ? ta + tint : T;
                const double ref = time[ta] + 0.5 * (time[tb - 1] - time[ta]);
                e = dl_phasor(r0 + (double)k * drate, time[t] - ref);
            }
            Et[2 * m] = e.x, Et[2 * m + 1] = -e.y;
        } else if (i < nF + nT + T) {
            const int s = (int)(i - nF - nT);  // tref[T]: I values, then zeros
            double ref = 0.0;
            if (valid && s < I) {
                const int ta = s * tint, tb = ta + tint < T ? ta + tint : T;
                ref = time[ta] + 0.5 * (time[tb - 1] - time[ta]);
            }
            tref[s] = ref;
        } else if (i < nF + nT + T + F) {
            const int f = (int)(i - nF - nT - T);
            af[f] = valid ? freq[f] - nu0 : 0.0;
        } else {
            const int t = (int)(i - nF - nT - T - F);
            double v = 0.0;
            if (valid) {
                const int ta = (t / tint) * tint, tb = ta + tint < T ? ta + tint : T;
                v = time[t] - (time[ta] + 0.5 * (time[tb - 1] - time[ta]));
            }
            dtm[t] = v;
        }
    }
}

struct FrSearch : DlSearch {
    // mode 0: the cells [j0, j1) x [k0, k1); 1: those within (wj, wk) of the grid's zero; 2: the whole grid, j1 = Nd, k1 = Nr
    int j0, j1, k0, k1, wj, wk;
    int ntiles;  // the delay tiles launched: cand is [B][Ib][ntiles][4]
    __device__ bool fits() const;
};

// the cells of a search; false: the call does not fit the table
__device__ __forceinline__ bool fr_window(const FrHead &h, const FrSearch &a, int *j0, int *j1, int *k0, int *k1)
{
    if (!h.ok || h.I != a.Ib) return false;
    if (a.mode == 1) {
        double zj = rint(-h.tau0 / h.dtau), zk = rint(-h.r0 / h.drate);
        zj = zj > 0.0 ? zj : 0.0, zk = zk > 0.0 ? zk : 0.0;  // (a NaN goes to 0)
        const int cj = zj < (double)(h.Nd - 1) ? (int)zj : h.Nd - 1, ck = zk < (double)(h.Nr - 1) ? (int)zk : h.Nr - 1;
        *j0 = cj - a.wj > 0 ? cj - a.wj : 0, *j1 = cj + a.wj + 1 < h.Nd ? cj + a.wj + 1 : h.Nd;
        *k0 = ck - a.wk > 0 ? ck - a.wk : 0, *k1 = ck + a.wk + 1 < h.Nr ? ck + a.wk + 1 : h.Nr;
    } else {
        *j0 = a.j0, *j1 = a.j1, *k0 = a.k0, *k1 = a.k1;
        if (a.mode == 2 && (a.j1 != h.Nd || a.k1 != h.Nr)) return false;
    }
    return *j0 >= 0 && *j0 < *j1 && *j1 <= h.Nd && *k0 >= 0 && *k0 < *k1 && *k1 <= h.Nr &&
           (*j1 - *j0 + FR_TJ - 1) / FR_TJ <= a.ntiles;
}

__device__ __forceinline__ bool FrSearch::fits() const
{
    int j0, j1, k0, k1;
    return fr_window(fr_head(tables, T, F), *this, &j0, &j1, &k0, &k1);
}

// X' of the sample at `at`: dl_sample's, derotated as ((x conj(d)) conj(Df)) conj(Dt)
__device__ __forceinline__ double2 fr_sample(const FrSearch &a, int64_t at, double2 d, double2 df, double2 dt, bool *flagged)
{
    return dl_sample(a, at, flagged, [&](double2 x) { return a.sol ? dl_mulc(dl_mulc(dl_mulc(x, d), df), dt) : x; });
}

// d_b, and Df and Dt of one (baseline, interval) into LDS (only with a solution); the caller puts a barrier behind it
__device__ __forceinline__ double2 fr_derotation(const FrSearch &a, const FrHead &h, int i, int p, int q, int t0, int nt,
                                                 double2 *Dfs, double2 *Dts, int tid, int nthreads)
{
    if (!a.sol) return make_double2(1.0, 0.0);
    const double *sp = a.sol + ((int64_t)i * a.A + p) * 4, *sq = a.sol + ((int64_t)i * a.A + q) * 4;
    const double dtau = sp[0] - sq[0], drate = sp[1] - sq[1];
    for (int f = tid; f < h.F; f += nthreads) Dfs[f] = dl_phasor(dtau, h.af[f]);
    for (int t = tid; t < nt; t += nthreads) Dts[t] = dl_phasor(drate, h.dtm[t0 + t]);
    return dl_mulc(make_double2(sp[2], sp[3]), make_double2(sq[2], sq[3]));
}

__global__ void __launch_bounds__(FR_THREADS) fr_search_kernel(FrSearch a)
{
    __shared__ double2 Xs[FR_MAX_TINT * FR_KC];  // X'[t][kc] of a chunk; then Y[t][jj]
    __shared__ double2 Es[FR_KC * FR_TJ];
    __shared__ double2 Dfs[FR_MAX_F], Dts[FR_MAX_TINT];
    __shared__ double rp[FR_THREADS / 64];
    __shared__ int rj[FR_THREADS / 64], rk[FR_THREADS / 64];
    const FrHead h = fr_head(a.tables, a.T, a.F);
    int j0, j1, k0, k1;
    if (!fr_window(h, a, &j0, &j1, &k0, &k1)) return;
    const int tid = threadIdx.x, tx = tid % FR_TJ, ty = tid / FR_TJ;
    const int b = (int)(blockIdx.x / (unsigned)a.ntiles), tile = (int)(blockIdx.x % (unsigned)a.ntiles);
    const int jt0 = j0 + tile * FR_TJ, j = jt0 + tx;
    const int64_t p = a.a1[b], q = a.a2[b];
    const bool live = jt0 < j1 && p >= 0 && p < a.A && q >= 0 && q < a.A && p != q;
    if (!live) {  // (the same for every thread)
        for (int i = tid; i < h.I; i += FR_THREADS) dl_put_cand(a.cand + (((int64_t)b * a.Ib + i) * a.ntiles + tile) * 4, -1.0, -1, -1);
        return;
    }
    double2 *Ys = Xs;
    for (int i = 0; i < h.I; ++i) {
        const int t0 = i * h.tint, nt = h.T - t0 < h.tint ? h.T - t0 : h.tint;
        __syncthreads();  // (the interval before has been read)
        const double2 d = fr_derotation(a, h, i, (int)p, (int)q, t0, nt, Dfs, Dts, tid, FR_THREADS);
        double2 acc[FR_NT];
#pragma unroll
        for (int r = 0; r < FR_NT; ++r) acc[r] = make_double2(0.0, 0.0);
        for (int c0 = 0; c0 < h.F; c0 += FR_KC) {
            const int nk = h.F - c0 < FR_KC ? h.F - c0 : FR_KC;
            __syncthreads();  // (Dfs and Dts are there; the chunk before has been read)
            for (int idx = tid; idx < nt * FR_KC; idx += FR_THREADS) {
                const int t = idx / FR_KC, kc = idx % FR_KC;
                double2 x = make_double2(0.0, 0.0);
                if (kc < nk) {
                    bool fl;
                    const double2 one = make_double2(1.0, 0.0);
                    x = fr_sample(a, ((int64_t)b * h.T + t0 + t) * h.F + c0 + kc, d, a.sol ? Dfs[c0 + kc] : one,
                                  a.sol ? Dts[t] : one, &fl);
                }
                Xs[idx] = x;
            }
            if (tid < FR_KC * FR_TJ) {
                const int kc = tid / FR_TJ, jj = tid % FR_TJ;
                Es[tid] = kc < nk && jt0 + jj < j1 ? h.Ef[(int64_t)(c0 + kc) * h.Nd + jt0 + jj] : make_double2(0.0, 0.0);
            }
            __syncthreads();
            for (int kc = 0; kc < nk; ++kc) {
                const double2 e = Es[kc * FR_TJ + tx];
#pragma unroll
                for (int r = 0; r < FR_NT; ++r) {
                    const int t = r * FR_TR + ty;
                    if (t < nt) dl_mac(acc[r], e, Xs[t * FR_KC + kc]);
                }
            }
        }
        __syncthreads();  // (the last chunk has been read)
#pragma unroll
        for (int r = 0; r < FR_NT; ++r) {
            const int t = r * FR_TR + ty;
            if (t < nt) Ys[t * FR_TJ + tx] = acc[r];
        }
        __syncthreads();
        double bp = -1.0;
        int bj = -1, bk = -1;
        if (j < j1) {
            for (int k = k0 + ty; k < k1; k += FR_TR) {
                double2 s = make_double2(0.0, 0.0);
                for (int t = 0; t < nt; ++t) dl_mac(s, h.Et[(int64_t)(t0 + t) * h.Nr + k], Ys[t * FR_TJ + tx]);
                const double P = s.x * s.x + s.y * s.y;
                if (P > bp) bp = P, bj = j, bk = k;  // (k ascends: the lowest k of equal powers stays)
            }
        }
        dl_group_best<FR_THREADS / 64>(tid, bp, bj, bk, rp, rj, rk);  // (the barrier at the head of the loop is between two uses)
        if (tid == 0) dl_put_cand(a.cand + (((int64_t)b * a.Ib + i) * a.ntiles + tile) * 4, bp, bj, bk);
    }
}

__global__ void __launch_bounds__(64) fr_refine_kernel(FrSearch a)
{
    __shared__ double2 Dfs[FR_MAX_F], Dts[FR_MAX_TINT];
    __shared__ double2 Ys[3][FR_MAX_TINT];
    __shared__ double es[FR_MAX_TINT];
    const FrHead h = fr_head(a.tables, a.T, a.F);
    int j0, j1, k0, k1;
    if (!fr_window(h, a, &j0, &j1, &k0, &k1)) return;
    const int lane = threadIdx.x;
    const int b = (int)(blockIdx.x / (unsigned)h.I), i = (int)(blockIdx.x % (unsigned)h.I);
    if (b >= a.B) return;
    double *row = a.peaks + ((int64_t)b * h.I + i) * FR_ROW;
    const int64_t p = a.a1[b], q = a.a2[b];
    int code = 0;
    double out[FR_ROW] = {};
    dl_row_none(out);
    u64 nflag = 0;
    if (!(p >= 0 && p < a.A && q >= 0 && q < a.A && p != q)) {
        code = 3;
    } else {
        const int t0 = i * h.tint, nt = h.T - t0 < h.tint ? h.T - t0 : h.tint;
        const double2 d = fr_derotation(a, h, i, (int)p, (int)q, t0, nt, Dfs, Dts, lane, 64);
        __syncthreads();
        const double2 one = make_double2(1.0, 0.0);
        // the energy and the counts: a lane owns the time steps lane, lane + 64, ...
        int nu = 0, nf = 0;
        bool bad = false;
        for (int t = lane; t < nt; t += 64) {
            double e = 0.0;
            for (int f = 0; f < h.F; ++f) {
                bool fl;
                const double2 x = fr_sample(a, ((int64_t)b * h.T + t0 + t) * h.F + f, d, a.sol ? Dfs[f] : one, a.sol ? Dts[t] : one, &fl);
                if (fl) {
                    ++nf;
                } else {
                    ++nu;
                    bad = bad || !(dl_finite(x.x) && dl_finite(x.y));
                    e = e + (x.x * x.x + x.y * x.y);
                }
            }
            es[t] = e;
        }
        for (int o = 32; o > 0; o >>= 1) nu += __shfl_xor(nu, o), nf += __shfl_xor(nf, o);
        bad = __any(bad);
        nflag = (u64)nf;
        // the best candidate over the delay tiles of the window
        double bp;
        int bj, bk;
        dl_best_tile(a.cand + ((int64_t)b * a.Ib + i) * a.ntiles * 4, (j1 - j0 + FR_TJ - 1) / FR_TJ, 1, 1, &bp, &bj, &bk);
        out[8] = (double)nu;
        if (nu == 0) {
            code = 1;
        } else if (bad || bj < j0 || bj >= j1 || bk < k0 || bk >= k1) {
            code = 2;
        } else {
            const bool inj = bj > j0 && bj < j1 - 1, ink = bk > k0 && bk < k1 - 1;
            __syncthreads();  // (es is there)
            for (int s = 0; s < 3; ++s) {
                if (s != 1 && !inj) continue;  // (the same for every lane)
                const int j = bj - 1 + s;
                for (int t = lane; t < nt; t += 64) {
                    double2 y = make_double2(0.0, 0.0);
                    for (int f = 0; f < h.F; ++f) {
                        bool fl;
                        const double2 x = fr_sample(a, ((int64_t)b * h.T + t0 + t) * h.F + f, d, a.sol ? Dfs[f] : one,
                                                    a.sol ? Dts[t] : one, &fl);
                        dl_mac(y, h.Ef[(int64_t)f * h.Nd + j], x);
                    }
                    Ys[s][t] = y;
                }
            }
            __syncthreads();
            // lane 0: (j*, k*); 1, 2: j* -+ 1; 3, 4: k* -+ 1
            double2 S = make_double2(0.0, 0.0);
            const bool mine = lane == 0 || ((lane == 1 || lane == 2) && inj) || ((lane == 3 || lane == 4) && ink);
            if (mine) {
                const int s = lane == 1 ? 0 : lane == 2 ? 2 : 1, k = lane == 3 ? bk - 1 : lane == 4 ? bk + 1 : bk;
                for (int t = 0; t < nt; ++t) dl_mac(S, h.Et[(int64_t)(t0 + t) * h.Nr + k], Ys[s][t]);
            }
            double N = 0.0;
            for (int t = 0; t < nt; ++t) N = N + es[t];
            // (the recomputed power of a selected cell is the candidate's: never a NaN)
            if (!dl_peak_row(out, bj, bk, inj, ink, S, N, nu, h.tau0, h.dtau, h.r0, h.drate)) code = 2;
        }
    }
    if (lane == 0) dl_put_row(a.cnt, row, out, code, nflag);
}

size_t fr_table_bytes(int64_t F, int64_t T, int64_t Nd, int64_t Nr) { return (size_t)GRIDHIP_FRINGE_TABLE_DOUBLES(F, T, Nd, Nr) * 8; }

int fr_tables_any(gridhip_ctx *ctx, bool dev, int64_t F, int64_t T, int64_t tint, const double *freq, const double *time,
                  double tau0, double dtau, int64_t Nd, double r0, double drate, int64_t Nr, double *tables)
{
    if (!ctx) return GRIDHIP_EINVAL;
    if (tint == 0) tint = T;
    if (F < 1 || F > FR_MAX_F || T < 1 || tint < 1 || tint > FR_MAX_TINT || Nd < 1 || Nd > FR_MAX_ND || Nr < 1 ||
        Nr > FR_MAX_NR || !freq || !time || !tables)
        return fail(ctx, GRIDHIP_EINVAL, "fringe_tables: bad argument");
    if (T > (1 << 20)) return fail(ctx, GRIDHIP_EUNSUPPORTED, "fringe_tables: T above 2^20");
    const size_t fb = (size_t)F * 8, tb = (size_t)T * 8, ab = fr_table_bytes(F, T, Nd, Nr);
    if (outputs_clash({{tables, ab}}, {{freq, fb}, {time, tb}}))
        return fail(ctx, GRIDHIP_EINVAL, "fringe_tables: arrays overlap");
    GH_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    Staged sg(ctx, dev);
    freq = sg.in(freq, fb), time = sg.in(time, tb), tables = sg.out(tables, ab);
    GH_CHECK(sg.status());
    hipLaunchKernelGGL(fr_head_kernel, dim3(1), dim3(256), 0, ctx->stream, (int)F, (int)T, (int)tint, (int)Nd, (int)Nr, freq,
                       time, tau0, dtau, r0, drate, tables);
    hipLaunchKernelGGL(fr_fill_kernel, grid_for(ctx, F * Nd + T * Nr + 2 * T + F), dim3(256), 0, ctx->stream, (int)F, (int)T,
                       (int)tint, (int)Nd, (int)Nr, freq, time, tables);
    GH_CHECK_HIP(ctx, hipGetLastError());
    return sg.finish();
}

struct FrMod {  // this module as delay_common.h's templates see it
    typedef FrSearch Search;
    typedef FrHead Head;
    static constexpr const char *fit_name = "fringefit", *apply_name = "apply_fringe";
    static constexpr int MAX_F = FR_MAX_F, MAX_N1 = FR_MAX_ND, MAX_N2 = FR_MAX_NR, MAX_ROUNDS = GRIDHIP_FRINGE_MAX_ROUNDS;

    static __device__ __forceinline__ FrHead head(const double *tb, int T, int F) { return fr_head(tb, T, F); }

    // v (d Df Dt) of the solutions sp and sq, or v conj(..): one factor after the other
    static __device__ __forceinline__ double2 rotate(const FrHead &h, int f, int t, const double *sp, const double *sq, int inverse,
                                                     double2 v)
    {
        const double2 d = dl_mulc(make_double2(sp[2], sp[3]), make_double2(sq[2], sq[3]));
        const double2 df = dl_phasor(sp[0] - sq[0], h.af[f]), dt = dl_phasor(sp[1] - sq[1], h.dtm[t]);
        return inverse ? dl_mulc(dl_mulc(dl_mulc(v, d), df), dt) : dl_mul(dl_mul(dl_mul(v, d), df), dt);
    }

    // (a table of other Nd or Nr has stopped the driver's whole-grid search: fr_window, mode 2)
    static __device__ __forceinline__ bool fit_steps(const double *tables, int T, int F, int I, int, int, double *d1, double *d2)
    {
        const FrHead h = fr_head(tables, T, F);
        *d1 = h.dtau, *d2 = h.drate;
        return h.ok && h.I == I;
    }

    static size_t table_bytes(int64_t F, int64_t T, int64_t Nd, int64_t Nr) { return fr_table_bytes(F, T, Nd, Nr); }

    static size_t host_table_bytes(const double *tables, int64_t T, int64_t F)
    {
        return dl_host_head_fits(tables, T, F, FR_MAX_TINT, FR_MAX_ND, FR_MAX_NR)
                   ? fr_table_bytes(F, T, (int64_t)tables[5], (int64_t)tables[6])
                   : (size_t)FR_HEAD * 8;
    }

    // (every field is set in every round: fr_window reads the half-widths in mode 1 alone and the cells in the other modes)
    static void round(FrSearch &a, bool whole, int64_t Nd, int64_t Nr, int64_t wj, int64_t wk)
    {
        a.mode = whole ? 2 : 1, a.j0 = 0, a.j1 = (int)Nd, a.k0 = 0, a.k1 = (int)Nr, a.wj = (int)wj, a.wk = (int)wk;
        a.ntiles = (int)(((whole ? Nd : 2 * wj + 1) + FR_TJ - 1) / FR_TJ);
    }
    static int64_t tiles(const FrSearch &a) { return a.ntiles; }
    static int64_t groups(const FrSearch &a, int64_t B, int64_t) { return B * a.ntiles; }
    static void search_launch(gridhip_ctx *ctx, const FrSearch &a, int64_t nI, double *stats)
    {
        hipLaunchKernelGGL(dl_zero_kernel, dim3(1), dim3(64), 0, ctx->stream, a.cnt);
        hipLaunchKernelGGL(fr_search_kernel, dim3((unsigned)groups(a, a.B, nI)), dim3(FR_THREADS), 0, ctx->stream, a);
        hipLaunchKernelGGL(fr_refine_kernel, dim3((unsigned)((int64_t)a.B * nI)), dim3(64), 0, ctx->stream, a);
        hipLaunchKernelGGL(dl_search_stats_kernel<FrSearch>, dim3(1), dim3(64), 0, ctx->stream, a, stats);
    }
};

int fr_search_any(gridhip_ctx *ctx, bool dev, int64_t B, int64_t T, int64_t F, int64_t A, int64_t I, const double *tables,
                  const double *vis, const double *model_vis, const double *wt, const int64_t *a1, const int64_t *a2,
                  const double *sol, int64_t j0, int64_t j1, int64_t k0, int64_t k1, double *peaks, double *stats)
{
    if (!ctx) return GRIDHIP_EINVAL;
    if (!dl_cube_ok(B, T, F, A, FR_MAX_F) || I < 1 || I > T || !tables || !vis || !a1 || !a2 || !peaks || !stats || j0 < 0 ||
        j0 >= j1 || j1 > FR_MAX_ND || k0 < 0 || k0 >= k1 || k1 > FR_MAX_NR || ((uintptr_t)vis & 15) || ((uintptr_t)model_vis & 15))
        return fail(ctx, GRIDHIP_EINVAL, "fringe_search: bad argument");
    if (!dl_cube_fits(B, T, A) || B * T > ((int64_t)1 << 31) - 1)
        return fail(ctx, GRIDHIP_EUNSUPPORTED, "fringe_search: B above 2^24, T above 2^20, A above 1024 or B T above 2^31 - 1");
    const size_t tb = dev ? (size_t)FR_HEAD * 8 : FrMod::host_table_bytes(tables, T, F);
    const int64_t ntiles = (j1 - j0 + FR_TJ - 1) / FR_TJ;
    if (B * ntiles > 0x7fffffffLL) return fail(ctx, GRIDHIP_EUNSUPPORTED, "fringe_search: more than 2^31 - 1 delay tiles");
    const size_t n = (size_t)B * T * F, pb = (size_t)B * I * FR_ROW * 8, sb = (size_t)I * A * 32, ib = (size_t)B * 8;
    if (outputs_clash({{peaks, pb}, {stats, 64}},
                      {{tables, tb}, {vis, n * 16}, {model_vis, n * 16}, {wt, n * 8}, {a1, ib}, {a2, ib}, {sol, sb}}))
        return fail(ctx, GRIDHIP_EINVAL, "fringe_search: arrays overlap");
    GH_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    DevBuf cnt, cand;
    GH_CHECK(cnt.alloc(ctx, sizeof(DlCount)));
    GH_CHECK(cand.alloc(ctx, (size_t)B * I * ntiles * 32));
    Staged sg(ctx, dev);
    FrSearch a{};
    dl_stage_search(sg, a, B, T, F, A, I, tables, tb, vis, model_vis, wt, a1, a2, peaks, cand, cnt);
    a.sol = sg.in(sol, sb);
    stats = sg.out(stats, 64);
    a.mode = 0, a.j0 = (int)j0, a.j1 = (int)j1, a.k0 = (int)k0, a.k1 = (int)k1, a.ntiles = (int)ntiles;
    GH_CHECK(sg.status());
    FrMod::search_launch(ctx, a, I, stats);
    GH_CHECK_HIP(ctx, hipGetLastError());
    return sg.finish();
}

}  // namespace

}  // namespace gridhip

using namespace gridhip;

extern "C" {

int gridhip_fringe_tables(gridhip_ctx *ctx, int64_t F, int64_t T, int64_t tint, const double *freq, const double *time,
                          double tau0, double dtau, int64_t Nd, double r0, double drate, int64_t Nr, double *tables)
{
    return fr_tables_any(ctx, false, F, T, tint, freq, time, tau0, dtau, Nd, r0, drate, Nr, tables);
}

int gridhip_fringe_tables_dev(gridhip_ctx *ctx, int64_t F, int64_t T, int64_t tint, const double *freq, const double *time,
                              double tau0, double dtau, int64_t Nd, double r0, double drate, int64_t Nr, double *tables)
{
    return fr_tables_any(ctx, true, F, T, tint, freq, time, tau0, dtau, Nd, r0, drate, Nr, tables);
}

int gridhip_fringe_search(gridhip_ctx *ctx, int64_t B, int64_t T, int64_t F, int64_t A, int64_t I, const double *tables,
                          const double *vis, const double *model_vis, const double *wt, const int64_t *a1, const int64_t *a2,
                          const double *sol, int64_t j0, int64_t j1, int64_t k0, int64_t k1, double *peaks, double *stats)
{
    return fr_search_any(ctx, false, B, T, F, A, I, tables, vis, model_vis, wt, a1, a2, sol, j0, j1, k0, k1, peaks, stats);
}

int gridhip_fringe_search_dev(gridhip_ctx *ctx, int64_t B, int64_t T, int64_t F, int64_t A, int64_t I, const double *tables,
                              const double *vis, const double *model_vis, const double *wt, const int64_t *a1,
                              const int64_t *a2, const double *sol, int64_t j0, int64_t j1, int64_t k0, int64_t k1,
                              double *peaks, double *stats)
{
    return fr_search_any(ctx, true, B, T, F, A, I, tables, vis, model_vis, wt, a1, a2, sol, j0, j1, k0, k1, peaks, stats);
}

int gridhip_fringefit(gridhip_ctx *ctx, int64_t B, int64_t T, int64_t F, int64_t A, int64_t I, int64_t Nd, int64_t Nr,
                      const double *tables, const double *vis, const double *model_vis, const double *wt, const int64_t *a1,
                      const int64_t *a2, int64_t rounds, int64_t wj, int64_t wk, double min_count, double min_coh2,
                      int64_t refant, int64_t niter, double tol, int warm, double *sol, double *peaks, double *info,
                      double *stats)
{
    return dl_fit_any<FrMod>(ctx, false, B, T, F, A, I, Nd, Nr, tables, vis, model_vis, wt, a1, a2, rounds, wj, wk, min_count,
                             min_coh2, refant, niter, tol, warm, sol, peaks, info, stats);
}

int gridhip_fringefit_dev(gridhip_ctx *ctx, int64_t B, int64_t T, int64_t F, int64_t A, int64_t I, int64_t Nd, int64_t Nr,
                          const double *tables, const double *vis, const double *model_vis, const double *wt,
                          const int64_t *a1, const int64_t *a2, int64_t rounds, int64_t wj, int64_t wk, double min_count,
                          double min_coh2, int64_t refant, int64_t niter, double tol, int warm, double *sol, double *peaks,
                          double *info, double *stats)
{
    return dl_fit_any<FrMod>(ctx, true, B, T, F, A, I, Nd, Nr, tables, vis, model_vis, wt, a1, a2, rounds, wj, wk, min_count,
                             min_coh2, refant, niter, tol, warm, sol, peaks, info, stats);
}

int gridhip_apply_fringe(gridhip_ctx *ctx, int64_t B, int64_t T, int64_t F, int64_t A, int64_t I, const double *tables,
                         const double *sol, const int64_t *a1, const int64_t *a2, int inverse, const double *vis_in,
                         const double *wt_in, double *vis_out, double *wt_out)
{
    return dl_apply_any<FrMod>(ctx, false, B, T, F, A, I, tables, sol, a1, a2, inverse, vis_in, wt_in, vis_out, wt_out);
}

int gridhip_apply_fringe_dev(gridhip_ctx *ctx, int64_t B, int64_t T, int64_t F, int64_t A, int64_t I, const double *tables,
                             const double *sol, const int64_t *a1, const int64_t *a2, int inverse, const double *vis_in,
                             const double *wt_in, double *vis_out, double *wt_out)
{
    return dl_apply_any<FrMod>(ctx, true, B, T, F, A, I, tables, sol, a1, a2, inverse, vis_in, wt_in, vis_out, wt_out);
}

int gridhip_fringe_tile(int64_t *out)
{
    if (!out) return GRIDHIP_EINVAL;
    out[0] = FR_TJ, out[1] = FR_KC, out[2] = FR_TR;
    return GRIDHIP_OK;
}

}  // extern "C"
