// Delay and rate calibration (include/gridhip.h, "delay and rate calibration"): a fringe search per baseline and solution
// interval over a grid of delays and rates, an antenna-based fit of the baseline values, and the apply step.
//
//     gridhip_fringe_tables   fr_head_kernel (one thread: the checks, the head), fr_fill_kernel (one thread per entry)
//     gridhip_fringe_search   fr_zero_kernel, fr_search_kernel, fr_refine_kernel, fr_search_stats_kernel
//     gridhip_fringe_solve    fr_solve_kernel (one work-group per interval), fr_solve_stats_kernel
//     gridhip_fringefit       [fr_init_sol_kernel]; per round the six above; fr_fit_stats_kernel
//     gridhip_apply_fringe    fr_apply_kernel (one thread per sample)
// Every kernel that reads a table judges its head itself and leaves at once when it does not fit the call; nothing is
// read back and the stop test of the solve is inside its kernel, so every _dev form is a fixed chain of launches.
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
// THE SOLVE KERNEL.  One work-group per interval; an antenna belongs to one thread.  The baselines pass through LDS twice
// in chunks of 256, once to count and once to fill, which leaves every antenna the list of its used baselines in ascending
// order in scratch; a Jacobi sweep reads only an antenna's own list, in that order: no floating-point atomic.
#include "common.h"
#include "fringe_solve.h"
#include "imaging.h"

#pragma clang fp contract(off)

namespace gridhip {

namespace {

typedef unsigned long long u64;

constexpr int FR_THREADS = 256;
constexpr int FR_TJ = 8;                     // delays of a work-group
constexpr int FR_KC = 8;                     // channels of a staged chunk
constexpr int FR_TR = FR_THREADS / FR_TJ;    // rates of a lane-pass, and the time steps of a pass of the first sum
constexpr int FR_HEAD = GRIDHIP_FRINGE_HEAD, FR_ROW = GRIDHIP_FRINGE_PEAK;
constexpr int FR_MAX_F = GRIDHIP_FRINGE_MAX_CHANNELS, FR_MAX_ND = GRIDHIP_FRINGE_MAX_DELAYS;
constexpr int FR_MAX_TINT = GRIDHIP_FRINGE_MAX_TINT, FR_MAX_NR = GRIDHIP_FRINGE_MAX_RATES;
constexpr int FR_MAX_A = GRIDHIP_FRINGE_MAX_ANTENNAS;
constexpr int FR_NT = FR_MAX_TINT / FR_TR;   // accumulators of a lane in the first sum
constexpr int FR_NA = FR_MAX_A / FR_THREADS; // antennas of a thread in the solve
static_assert(FR_TJ * FR_KC <= FR_THREADS && FR_NT * FR_TR == FR_MAX_TINT, "the search kernel's staging");

struct FrCount {  // the counters of one search
    u64 flagged, bad, empty, refused, ok;
    u64 pad[3];
};

struct FrHead {
    bool ok;
    int F, T, tint, I, Nd, Nr;
    double tau0, dtau, r0, drate;
    const double2 *Ef, *Et;
    const double *tref, *af, *dtm;
};

__device__ __forceinline__ bool fr_finite(double x) { return __builtin_isfinite(x); }

__device__ __forceinline__ bool fr_int_in(double v, int lo, int hi) { return v >= (double)lo && v <= (double)hi && v == (double)(int)v; }

// the head of a table, and whether it fits a cube of T time steps and F channels
__device__ __forceinline__ FrHead fr_head(const double *tb, int T, int F)
{
    FrHead h;
    h.ok = tb[0] == 1.0 && tb[1] == (double)F && tb[2] == (double)T && fr_int_in(tb[3], 1, FR_MAX_TINT) &&
           fr_int_in(tb[5], 1, FR_MAX_ND) && fr_int_in(tb[6], 1, FR_MAX_NR) && F >= 1 && F <= FR_MAX_F && T >= 1;
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

// exp(2 pi i a b) = (cs, sn): the turns x = a * b reduced to x - rint(x) (exact), then sincospi of twice that
__device__ __forceinline__ double2 fr_phasor(double a, double b)
{
    const double x = a * b;
    const double r = x - rint(x);
    double sn, cs;
    sincospi(2.0 * r, &sn, &cs);
    return make_double2(cs, sn);
}

// x conj(c): four rounded products, two rounded sums
__device__ __forceinline__ double2 fr_mulc(double2 x, double2 c) { return make_double2(x.x * c.x + x.y * c.y, x.y * c.x - x.x * c.y); }
// x c
__device__ __forceinline__ double2 fr_mul(double2 x, double2 c) { return make_double2(x.x * c.x - x.y * c.y, x.x * c.y + x.y * c.x); }
// acc + e x as rmsynth adds it
__device__ __forceinline__ void fr_mac(double2 &acc, double2 e, double2 x)
{
    acc.x = acc.x + (e.x * x.x - e.y * x.y);
    acc.y = acc.y + (e.x * x.y + e.y * x.x);
}

__global__ void __launch_bounds__(256)
    fr_head_kernel(int F, int T, int tint, int Nd, int Nr, const double *__restrict__ freq, const double *__restrict__ time,
                   double tau0, double dtau, double r0, double drate, double *__restrict__ tables)
{
    if (blockIdx.x != 0) return;
    int bad = 0;  // the one work-group shares the scan of freq and time
    for (int i = threadIdx.x; i < F + T; i += blockDim.x) bad |= !fr_finite(i < F ? freq[i] : time[i - F]);
    bad = __syncthreads_or(bad);
    if (threadIdx.x != 0) return;
    const double nu0 = freq[0] + 0.5 * (freq[F - 1] - freq[0]);
    const bool ok = !bad && fr_finite(tau0) && fr_finite(dtau) && fr_finite(r0) && fr_finite(drate) && dtau > 0.0 &&
                    drate > 0.0 && fr_finite(nu0);
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
                e = fr_phasor(tau0 + (double)j * dtau, freq[f] - nu0);
            }
            Ef[2 * i] = e.x, Ef[2 * i + 1] = -e.y;
        } else if (i < nF + nT) {
            const int64_t m = i - nF;
            double2 e = make_double2(0.0, 0.0);
            if (valid) {
                const int t = (int)(m / Nr), k = (int)(m % Nr);
                const int ta = (t / tint) * tint, tb = ta + tint < T ? ta + tint : T;
                const double ref = time[ta] + 0.5 * (time[tb - 1] - time[ta]);
                e = fr_phasor(r0 + (double)k * drate, time[t] - ref);
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

struct FrSearch {
    int B, T, F, A;
    const double *tables;
    const double2 *vis, *model;
    const double *wt;
    const int64_t *a1, *a2;
    const double *sol;
    int mode;  // 0: the cells [j0, j1) x [k0, k1); 1: those within (wj, wk) of the grid's zero; 2: the whole grid, j1 = Nd, k1 = Nr
    int j0, j1, k0, k1, wj, wk;
    int ntiles, Ib;  // the delay tiles launched, and the caller's I: the table's, or the call does not fit
    double *cand;    // [B][Ib][ntiles][4] = { P, j, k, 0 }, P = -1: none
    double *peaks;
    FrCount *cnt;
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

// X' of the sample at `at`; *flagged: its weight is not > 0 and it is (0, 0)
__device__ __forceinline__ double2 fr_sample(const FrSearch &a, int64_t at, double2 d, double2 df, double2 dt, bool *flagged)
{
    const double s = a.wt ? a.wt[at] : 1.0;
    *flagged = !(s > 0.0);
    if (*flagged) return make_double2(0.0, 0.0);
    const double2 v = a.vis[at];
    double2 x = make_double2(s * v.x, s * v.y);
    if (a.model) x = fr_mulc(x, a.model[at]);
    if (a.sol) x = fr_mulc(fr_mulc(fr_mulc(x, d), df), dt);
    return x;
}

// d_b, and Df and Dt of one (baseline, interval) into LDS (only with a solution); the caller puts a barrier behind it
__device__ __forceinline__ double2 fr_derotation(const FrSearch &a, const FrHead &h, int i, int p, int q, int t0, int nt,
                                                 double2 *Dfs, double2 *Dts, int tid, int nthreads)
{
    if (!a.sol) return make_double2(1.0, 0.0);
    const double *sp = a.sol + ((int64_t)i * a.A + p) * 4, *sq = a.sol + ((int64_t)i * a.A + q) * 4;
    const double dtau = sp[0] - sq[0], drate = sp[1] - sq[1];
    for (int f = tid; f < h.F; f += nthreads) Dfs[f] = fr_phasor(dtau, h.af[f]);
    for (int t = tid; t < nt; t += nthreads) Dts[t] = fr_phasor(drate, h.dtm[t0 + t]);
    return fr_mulc(make_double2(sp[2], sp[3]), make_double2(sq[2], sq[3]));
}

// is (q, qj, qk) ahead of (p, pj, pk)?  The largest power, then the lowest delay, then the lowest rate; a "none"
// (-1, -1, -1) is behind everything
__device__ __forceinline__ bool fr_ahead(double q, int qj, int qk, double p, int pj, int pk)
{
    return q > p || (q == p && (qj < pj || (qj == pj && qk < pk)));
}

__global__ void fr_zero_kernel(FrCount *cnt)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) *cnt = FrCount{};
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
        for (int i = tid; i < h.I; i += FR_THREADS) {
            double *c = a.cand + (((int64_t)b * a.Ib + i) * a.ntiles + tile) * 4;
            c[0] = -1.0, c[1] = -1.0, c[2] = -1.0, c[3] = 0.0;
        }
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
                    if (t < nt) fr_mac(acc[r], e, Xs[t * FR_KC + kc]);
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
                for (int t = 0; t < nt; ++t) fr_mac(s, h.Et[(int64_t)(t0 + t) * h.Nr + k], Ys[t * FR_TJ + tx]);
                const double P = s.x * s.x + s.y * s.y;
                if (P > bp) bp = P, bj = j, bk = k;  // (k ascends: the lowest k of equal powers stays)
            }
        }
        for (int o = 32; o > 0; o >>= 1) {
            const double qp = __shfl_xor(bp, o);
            const int qj = __shfl_xor(bj, o), qk = __shfl_xor(bk, o);
            if (fr_ahead(qp, qj, qk, bp, bj, bk)) bp = qp, bj = qj, bk = qk;
        }
        if ((tid & 63) == 0) rp[tid >> 6] = bp, rj[tid >> 6] = bj, rk[tid >> 6] = bk;
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < FR_THREADS / 64; ++w)
                if (fr_ahead(rp[w], rj[w], rk[w], bp, bj, bk)) bp = rp[w], bj = rj[w], bk = rk[w];
            double *c = a.cand + (((int64_t)b * a.Ib + i) * a.ntiles + tile) * 4;
            c[0] = bp, c[1] = (double)bj, c[2] = (double)bk, c[3] = 0.0;
        }
    }
}

// the second half of the parabola rule of gridhip_rmclean: the offset in cells from the three powers, 0 where it does not apply
__device__ __forceinline__ double fr_parabola(double pm, double ps, double pp)
{
    const double d = (pm - ps) + (pp - ps);
    return d < 0.0 ? (0.5 * (pm - pp)) / d : 0.0;
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
    double out[FR_ROW] = {-1.0, -1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
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
                    bad = bad || !(fr_finite(x.x) && fr_finite(x.y));
                    e = e + (x.x * x.x + x.y * x.y);
                }
            }
            es[t] = e;
        }
        for (int o = 32; o > 0; o >>= 1) nu += __shfl_xor(nu, o), nf += __shfl_xor(nf, o);
        bad = __any(bad);
        nflag = (u64)nf;
        // the best candidate, tiles ascending
        double bp = -1.0;
        int bj = -1, bk = -1;
        const int ntl = (j1 - j0 + FR_TJ - 1) / FR_TJ;
        for (int tl = 0; tl < ntl; ++tl) {
            const double *c = a.cand + (((int64_t)b * a.Ib + i) * a.ntiles + tl) * 4;
            const double cp = c[0];
            if (cp > bp) bp = cp, bj = (int)c[1], bk = (int)c[2];  // (the delays ascend with the tiles)
        }
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
                        fr_mac(y, h.Ef[(int64_t)f * h.Nd + j], x);
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
                for (int t = 0; t < nt; ++t) fr_mac(S, h.Et[(int64_t)(t0 + t) * h.Nr + k], Ys[s][t]);
            }
            const double P = S.x * S.x + S.y * S.y;
            const double ps = __shfl(P, 0), pjm = __shfl(P, 1), pjp = __shfl(P, 2), pkm = __shfl(P, 3), pkp = __shfl(P, 4);
            const double sre = __shfl(S.x, 0), sim = __shfl(S.y, 0);
            double N = 0.0;
            for (int t = 0; t < nt; ++t) N = N + es[t];
            double tau = h.tau0 + (double)bj * h.dtau, rate = h.r0 + (double)bk * h.drate;
            if (inj) tau = tau + fr_parabola(pjm, ps, pjp) * h.dtau;
            if (ink) rate = rate + fr_parabola(pkm, ps, pkp) * h.drate;
            out[0] = (double)bj, out[1] = (double)bk, out[2] = ps, out[3] = tau, out[4] = rate;
            if (ps > 0.0) {
                const double sq = sqrt(ps);
                out[5] = sre / sq, out[6] = sim / sq;
            }
            out[7] = N > 0.0 ? ps / ((double)nu * N) : 0.0;
            out[9] = N;
            if (!(ps == ps)) code = 2;  // (the recomputed power of a selected cell is the candidate's: never)
        }
    }
    if (lane == 0) {
        if (code != 0) {
            out[0] = -1.0, out[1] = -1.0, out[2] = 0.0, out[3] = 0.0, out[4] = 0.0, out[5] = 1.0, out[6] = 0.0, out[7] = 0.0;
            out[9] = 0.0;
        }
        out[10] = (double)code;
#pragma unroll
        for (int c = 0; c < FR_ROW; ++c) row[c] = out[c];
        if (nflag) atomicAdd(&a.cnt->flagged, nflag);
        atomicAdd(code == 0 ? &a.cnt->ok : code == 1 ? &a.cnt->empty : code == 2 ? &a.cnt->bad : &a.cnt->refused, (u64)1);
    }
}

__global__ void fr_search_stats_kernel(FrSearch a, double *__restrict__ stats)
{
    if (blockIdx.x != 0 || threadIdx.x != 0 || !stats) return;
    const FrHead h = fr_head(a.tables, a.T, a.F);
    int j0, j1, k0, k1;
    const bool ok = fr_window(h, a, &j0, &j1, &k0, &k1);
    for (int i = 0; i < GRIDHIP_FRINGE_STATS; ++i) stats[i] = 0.0;
    if (ok) {
        stats[0] = (double)a.cnt->flagged, stats[1] = (double)a.cnt->bad, stats[2] = (double)a.cnt->empty;
        stats[3] = (double)a.cnt->refused, stats[4] = (double)a.cnt->ok;
    } else {
        stats[7] = 1.0;
    }
}

// (FrEdge and FrSolve: fringe_solve.h)

// a chunk of FR_THREADS baselines of interval i into LDS: the pair, the weight (0 beyond B) and, with `rows`, the values
__device__ __forceinline__ void fr_solve_chunk(const FrSolve &a, int i, int c0, const double *w, bool rows, int *cp, int *cq,
                                               double (*cv)[FR_THREADS])
{
    const int tid = threadIdx.x, b = c0 + tid;
    double wb = 0.0;
    if (b < a.B) {
        wb = w[b];
        cp[tid] = (int)a.a1[b], cq[tid] = (int)a.a2[b];  // (a used baseline's pair is in range)
        if (rows && wb > 0.0) {
            const double *row = a.peaks + ((int64_t)b * a.I + i) * FR_ROW;
            cv[1][tid] = row[3], cv[2][tid] = row[4], cv[3][tid] = row[5], cv[4][tid] = row[6];
        }
    }
    cv[0][tid] = wb;
}

__global__ void __launch_bounds__(FR_THREADS) fr_solve_kernel(FrSolve a)
{
    __shared__ double xt[FR_MAX_A], xr[FR_MAX_A];
    __shared__ double2 hs[FR_MAX_A];
    __shared__ double red[FR_THREADS / 64][5];
    __shared__ double sums[3][FR_THREADS];
    __shared__ double cv[5][FR_THREADS];
    __shared__ int cp[FR_THREADS], cq[FR_THREADS];
    __shared__ int offs[FR_MAX_A + 1];
    __shared__ int cnts[2];
    const int tid = threadIdx.x, i = blockIdx.x, B = a.B, A = a.A;
    if (a.gate && a.gate[7] != 0.0) return;
    double *w = a.w + (int64_t)i * B;
    FrEdge *edges = a.edges + (int64_t)i * 2 * B;
    if (tid < 2) cnts[tid] = 0;
    for (int b = tid; b < B; b += FR_THREADS) {
        const double *row = a.peaks + ((int64_t)b * a.I + i) * FR_ROW;
        const int64_t p = a.a1[b], q = a.a2[b];
        const double coh2 = row[7];
        const bool use = row[10] == 0.0 && row[8] >= a.min_count && coh2 >= a.min_coh2 && coh2 > 0.0 && fr_finite(coh2) &&
                         fr_finite(row[3]) && fr_finite(row[4]) && fr_finite(row[5]) && fr_finite(row[6]) && p >= 0 && p < A &&
                         q >= 0 && q < A && p != q;
        w[b] = use ? coh2 : 0.0;
    }
    for (int s = tid; s < A; s += FR_THREADS) xt[s] = 0.0, xr[s] = 0.0, hs[s] = make_double2(1.0, 0.0);
    // the used baselines of every antenna, b ascending, as a list of its own: the baselines pass through LDS in chunks,
    // once to count and once to fill, and a sweep then reads only an antenna's own entries
    int cnt[FR_NA], pos[FR_NA];
#pragma unroll
    for (int r = 0; r < FR_NA; ++r) cnt[r] = 0;
    for (int c0 = 0; c0 < B; c0 += FR_THREADS) {
        __syncthreads();  // (w is there; the chunk before has been read)
        fr_solve_chunk(a, i, c0, w, false, cp, cq, cv);
        __syncthreads();
        const int n = B - c0 < FR_THREADS ? B - c0 : FR_THREADS;
#pragma unroll
        for (int r = 0; r < FR_NA; ++r) {
            const int s = tid + r * FR_THREADS;
            if (s < A)
                for (int k = 0; k < n; ++k)
                    if (cv[0][k] > 0.0 && (cp[k] == s || cq[k] == s)) ++cnt[r];
        }
    }
#pragma unroll
    for (int r = 0; r < FR_NA; ++r)
        if (tid + r * FR_THREADS < A) offs[tid + r * FR_THREADS + 1] = cnt[r];
    __syncthreads();
    if (tid == 0) {
        offs[0] = 0;
        for (int s = 0; s < A; ++s) offs[s + 1] += offs[s];  // (at most 2 B entries)
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < FR_NA; ++r) pos[r] = tid + r * FR_THREADS < A ? offs[tid + r * FR_THREADS] : 0;
    for (int c0 = 0; c0 < B; c0 += FR_THREADS) {
        __syncthreads();
        fr_solve_chunk(a, i, c0, w, true, cp, cq, cv);
        __syncthreads();
        const int n = B - c0 < FR_THREADS ? B - c0 : FR_THREADS;
#pragma unroll
        for (int r = 0; r < FR_NA; ++r) {
            const int s = tid + r * FR_THREADS;
            if (s < A)
                for (int k = 0; k < n; ++k)
                    if (cv[0][k] > 0.0 && (cp[k] == s || cq[k] == s)) {
                        FrEdge e;
                        e.w = cv[0][k], e.tau = cv[1][k], e.r = cv[2][k], e.zr = cv[3][k], e.zi = cv[4][k];
                        e.side = cp[k] == s ? 0 : 1, e.other = e.side ? cp[k] : cq[k];
                        edges[pos[r]++] = e;
                    }
        }
    }
    __syncthreads();
    int iters = 0;
    for (int it = 0; it < a.niter; ++it) {
        double nxt[FR_NA], nxr[FR_NA];
        double2 nh[FR_NA];
        double ct = 0.0, st = 0.0, cr = 0.0, sr = 0.0, ch = 0.0;
#pragma unroll
        for (int r = 0; r < FR_NA; ++r) {
            const int s = tid + r * FR_THREADS;
            if (s >= A || cnt[r] == 0) continue;
            double den = 0.0, nt = 0.0, nr = 0.0;
            double2 num = make_double2(0.0, 0.0);
            for (int k = offs[s]; k < offs[s + 1]; ++k) {
                const FrEdge e = edges[k];
                const double wb = e.w;
                const double2 wz = make_double2(wb * e.zr, wb * e.zi);
                const double2 g = hs[e.other];
                den = den + wb;
                if (e.side == 0) {
                    nt = nt + wb * (e.tau + xt[e.other]);
                    nr = nr + wb * (e.r + xr[e.other]);
                    num.x = num.x + (wz.x * g.x - wz.y * g.y);
                    num.y = num.y + (wz.x * g.y + wz.y * g.x);
                } else {
                    nt = nt + wb * (xt[e.other] - e.tau);
                    nr = nr + wb * (xr[e.other] - e.r);
                    num.x = num.x + (wz.x * g.x + wz.y * g.y);
                    num.y = num.y + (wz.x * g.y - wz.y * g.x);
                }
            }
            double t1 = nt / den, r1 = nr / den;
            double2 g1 = hs[s];
            const double m2 = num.x * num.x + num.y * num.y;
            if (m2 > 0.0 && fr_finite(m2)) {
                const double sq = sqrt(m2);
                g1 = make_double2(num.x / sq, num.y / sq);
            }
            if (it & 1) {
                t1 = 0.5 * (t1 + xt[s]), r1 = 0.5 * (r1 + xr[s]);
                const double2 av = make_double2(0.5 * (g1.x + hs[s].x), 0.5 * (g1.y + hs[s].y));
                const double n2 = av.x * av.x + av.y * av.y;
                if (n2 > 0.0 && fr_finite(n2)) {
                    const double sq = sqrt(n2);
                    g1 = make_double2(av.x / sq, av.y / sq);
                } else {
                    g1 = hs[s];
                }
            }
            nxt[r] = t1, nxr[r] = r1, nh[r] = g1;
            const double dx = g1.x - hs[s].x, dy = g1.y - hs[s].y;
            ct = fmax(ct, fabs(t1 - xt[s])), st = fmax(st, fabs(t1));
            cr = fmax(cr, fabs(r1 - xr[s])), sr = fmax(sr, fabs(r1));
            ch = fmax(ch, sqrt(dx * dx + dy * dy));
        }
        for (int o = 32; o > 0; o >>= 1) {
            ct = fmax(ct, __shfl_xor(ct, o)), st = fmax(st, __shfl_xor(st, o)), cr = fmax(cr, __shfl_xor(cr, o));
            sr = fmax(sr, __shfl_xor(sr, o)), ch = fmax(ch, __shfl_xor(ch, o));
        }
        __syncthreads();  // (every thread has read xt, xr, hs; red of the sweep before has been read)
        if ((tid & 63) == 0) red[tid >> 6][0] = ct, red[tid >> 6][1] = st, red[tid >> 6][2] = cr, red[tid >> 6][3] = sr, red[tid >> 6][4] = ch;
#pragma unroll
        for (int r = 0; r < FR_NA; ++r) {
            const int s = tid + r * FR_THREADS;
            if (s < A && cnt[r] != 0) xt[s] = nxt[r], xr[s] = nxr[r], hs[s] = nh[r];
        }
        __syncthreads();
        ++iters;
        for (int wv = 0; wv < FR_THREADS / 64; ++wv) {
            ct = fmax(ct, red[wv][0]), st = fmax(st, red[wv][1]), cr = fmax(cr, red[wv][2]);
            sr = fmax(sr, red[wv][3]), ch = fmax(ch, red[wv][4]);
        }
        if (ct <= a.tol * st && cr <= a.tol * sr && ch <= a.tol) break;  // (the same for every thread; a NaN goes on)
    }
    // reference, accumulate, info
    const bool refd = a.refant >= 0;
    bool ref_ok = false;
    double reft = 0.0, refr = 0.0;
    double2 refh = make_double2(1.0, 0.0);
    if (refd) {
        reft = xt[a.refant], refr = xr[a.refant], refh = hs[a.refant];
        const int c = offs[a.refant + 1] - offs[a.refant];
        ref_ok = c != 0;
    }
    __syncthreads();  // (the reference values have been read)
    int unsolved = 0;
#pragma unroll
    for (int r = 0; r < FR_NA; ++r) {
        const int s = tid + r * FR_THREADS;
        if (s >= A) continue;
        a.info[(int64_t)i * A + s] = (double)cnt[r];
        if (cnt[r] == 0) {
            ++unsolved;
            continue;
        }
        double t1 = xt[s], r1 = xr[s];
        double2 g1 = hs[s];
        if (ref_ok) {
            t1 = t1 - reft, r1 = r1 - refr;
            g1 = s == a.refant ? make_double2(1.0, 0.0) : fr_mulc(g1, refh);
        }
        double *so = a.sol + ((int64_t)i * A + s) * 4;
        so[0] = so[0] + t1, so[1] = so[1] + r1;
        const double2 g = fr_mul(make_double2(so[2], so[3]), g1);
        const double m2 = g.x * g.x + g.y * g.y;
        if (m2 > 0.0 && fr_finite(m2)) {
            const double sq = sqrt(m2);
            so[2] = g.x / sq, so[3] = g.y / sq;
        } else {
            so[2] = g.x, so[3] = g.y;
        }
    }
    // the interval's share of the stats: a thread adds a contiguous run of baselines in order, thread 0 the 256 runs
    const int run = (B + FR_THREADS - 1) / FR_THREADS;
    double sw = 0.0, swt = 0.0, swr = 0.0;
    int used = 0;
    for (int b = tid * run; b < B && b < (tid + 1) * run; ++b) {
        const double wb = w[b];
        if (!(wb > 0.0)) continue;
        const double *row = a.peaks + ((int64_t)b * a.I + i) * FR_ROW;
        ++used;
        sw = sw + wb, swt = swt + wb * (row[3] * row[3]), swr = swr + wb * (row[4] * row[4]);
    }
    sums[0][tid] = sw, sums[1][tid] = swt, sums[2][tid] = swr;
    if (used) atomicAdd(&cnts[0], used);
    if (unsolved) atomicAdd(&cnts[1], unsolved);
    __syncthreads();
    if (tid == 0) {
        sw = 0.0, swt = 0.0, swr = 0.0;
        for (int c = 0; c < FR_THREADS; ++c) sw = sw + sums[0][c], swt = swt + sums[1][c], swr = swr + sums[2][c];
        double *pt = a.part + (int64_t)i * 8;
        pt[0] = (double)iters, pt[1] = (double)cnts[0], pt[2] = (double)cnts[1], pt[3] = refd && !ref_ok ? 1.0 : 0.0;
        pt[4] = sw, pt[5] = swt, pt[6] = swr, pt[7] = 0.0;
    }
}

__global__ void fr_solve_stats_kernel(FrSolve a, double *__restrict__ stats)
{
    if (blockIdx.x != 0 || threadIdx.x != 0 || !stats) return;
    if (a.gate && a.gate[7] != 0.0) return;
    double it = 0.0, used = 0.0, uns = 0.0, noref = 0.0, sw = 0.0, swt = 0.0, swr = 0.0;
    for (int i = 0; i < a.I; ++i) {
        const double *pt = a.part + (int64_t)i * 8;
        it = pt[0] > it ? pt[0] : it;
        used = used + pt[1], uns = uns + pt[2], noref = noref + pt[3], sw = sw + pt[4], swt = swt + pt[5], swr = swr + pt[6];
    }
    stats[0] = it, stats[1] = used, stats[2] = uns, stats[3] = noref;
    stats[4] = sw > 0.0 ? sqrt(swt / sw) : 0.0, stats[5] = sw > 0.0 ? sqrt(swr / sw) : 0.0;
    stats[6] = 0.0, stats[7] = 0.0;
}

__global__ void fr_init_sol_kernel(int64_t n, double *__restrict__ sol)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) sol[4 * i] = 0.0, sol[4 * i + 1] = 0.0, sol[4 * i + 2] = 1.0, sol[4 * i + 3] = 0.0;
}

// the driver's stats from those of its last search and solve
__global__ void fr_fit_stats_kernel(int T, int F, int I, const double *__restrict__ tables, const double *__restrict__ ss,
                                    const double *__restrict__ vs, double *__restrict__ stats)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const FrHead h = fr_head(tables, T, F);
    for (int i = 0; i < GRIDHIP_FRINGE_STATS; ++i) stats[i] = 0.0;
    if (!h.ok || h.I != I || ss[7] != 0.0) {
        stats[7] = 1.0;
        return;
    }
    stats[0] = vs[0], stats[1] = ss[0], stats[2] = ss[1], stats[3] = ss[2], stats[4] = vs[2];
    stats[5] = vs[4] / h.dtau, stats[6] = vs[5] / h.drate;
}

struct FrApply {
    int B, T, F, A, I;
    const double *tables, *sol;
    const int64_t *a1, *a2;
    int inverse;
    const double2 *vis_in;
    const double *wt_in;
    double2 *vis_out;
    double *wt_out;
};

__global__ void __launch_bounds__(256) fr_apply_kernel(FrApply a)
{
    const FrHead h = fr_head(a.tables, a.T, a.F);
    if (!h.ok || h.I != a.I) return;
    const int64_t n = (int64_t)a.B * a.T * a.F;
    const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, step = (int64_t)gridDim.x * blockDim.x;
    for (int64_t at = i0; at < n; at += step) {
        const int f = (int)(at % a.F);
        const int64_t bt = at / a.F;
        const int t = (int)(bt % a.T), b = (int)(bt / a.T), i = t / h.tint;
        const int64_t p = a.a1[b], q = a.a2[b];
        double2 v = a.vis_in[at];
        double wv = a.wt_in ? a.wt_in[at] : 1.0;
        bool ok = p >= 0 && p < a.A && q >= 0 && q < a.A;
        if (ok) {
            const double *sp = a.sol + ((int64_t)i * a.A + p) * 4, *sq = a.sol + ((int64_t)i * a.A + q) * 4;
            ok = fr_finite(sp[0]) && fr_finite(sp[1]) && fr_finite(sp[2]) && fr_finite(sp[3]) && fr_finite(sq[0]) &&
                 fr_finite(sq[1]) && fr_finite(sq[2]) && fr_finite(sq[3]);
            if (ok) {
                const double2 d = fr_mulc(make_double2(sp[2], sp[3]), make_double2(sq[2], sq[3]));
                const double2 df = fr_phasor(sp[0] - sq[0], h.af[f]), dt = fr_phasor(sp[1] - sq[1], h.dtm[t]);
                v = a.inverse ? fr_mulc(fr_mulc(fr_mulc(v, d), df), dt) : fr_mul(fr_mul(fr_mul(v, d), df), dt);
            }
        }
        a.vis_out[at] = v;
        if (a.wt_out) a.wt_out[at] = ok ? wv : 0.0;
    }
}

size_t fr_table_bytes(int64_t F, int64_t T, int64_t Nd, int64_t Nr) { return (size_t)GRIDHIP_FRINGE_TABLE_DOUBLES(F, T, Nd, Nr) * 8; }

bool fr_cube_ok(int64_t B, int64_t T, int64_t F, int64_t A)
{
    return B >= 1 && T >= 1 && F >= 1 && F <= FR_MAX_F && A >= 2;
}

// EUNSUPPORTED beyond these: the kernels index baselines and time steps with 32 bits
bool fr_cube_fits(int64_t B, int64_t T, int64_t A) { return B <= (1 << 24) && T <= (1 << 20) && A <= FR_MAX_A; }

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

// the size of a host form's table, from its head in host memory: the whole table where the head fits the cube, else the
// head alone (the kernels see the same head and leave)
size_t fr_host_table_bytes(const double *tables, int64_t T, int64_t F)
{
    const double tint = tables[3], Nd = tables[5], Nr = tables[6];
    if (tables[0] == 1.0 && tables[1] == (double)F && tables[2] == (double)T && tint >= 1.0 && tint <= FR_MAX_TINT &&
        tint == (double)(int64_t)tint && Nd >= 1.0 && Nd <= FR_MAX_ND && Nd == (double)(int64_t)Nd && Nr >= 1.0 &&
        Nr <= FR_MAX_NR && Nr == (double)(int64_t)Nr)
        return fr_table_bytes(F, T, (int64_t)Nd, (int64_t)Nr);
    return (size_t)FR_HEAD * 8;
}

void fr_search_launch(gridhip_ctx *ctx, const FrSearch &a, int64_t nI, double *stats)
{
    hipLaunchKernelGGL(fr_zero_kernel, dim3(1), dim3(64), 0, ctx->stream, a.cnt);
    hipLaunchKernelGGL(fr_search_kernel, dim3((unsigned)((int64_t)a.B * a.ntiles)), dim3(FR_THREADS), 0, ctx->stream, a);
    hipLaunchKernelGGL(fr_refine_kernel, dim3((unsigned)((int64_t)a.B * nI)), dim3(64), 0, ctx->stream, a);
    hipLaunchKernelGGL(fr_search_stats_kernel, dim3(1), dim3(64), 0, ctx->stream, a, stats);
}

void fr_solve_launch(gridhip_ctx *ctx, const FrSolve &a, double *stats)
{
    hipLaunchKernelGGL(fr_solve_kernel, dim3((unsigned)a.I), dim3(FR_THREADS), 0, ctx->stream, a);
    hipLaunchKernelGGL(fr_solve_stats_kernel, dim3(1), dim3(64), 0, ctx->stream, a, stats);
}

int fr_search_any(gridhip_ctx *ctx, bool dev, int64_t B, int64_t T, int64_t F, int64_t A, int64_t I, const double *tables,
                  const double *vis, const double *model_vis, const double *wt, const int64_t *a1, const int64_t *a2,
                  const double *sol, int64_t j0, int64_t j1, int64_t k0, int64_t k1, double *peaks, double *stats)
{
    if (!ctx) return GRIDHIP_EINVAL;
    if (!fr_cube_ok(B, T, F, A) || I < 1 || I > T || !tables || !vis || !a1 || !a2 || !peaks || !stats || j0 < 0 || j0 >= j1 ||
        j1 > FR_MAX_ND || k0 < 0 || k0 >= k1 || k1 > FR_MAX_NR || ((uintptr_t)vis & 15) || ((uintptr_t)model_vis & 15))
        return fail(ctx, GRIDHIP_EINVAL, "fringe_search: bad argument");
    if (!fr_cube_fits(B, T, A) || B * T > ((int64_t)1 << 31) - 1)
        return fail(ctx, GRIDHIP_EUNSUPPORTED, "fringe_search: B above 2^24, T above 2^20, A above 1024 or B T above 2^31 - 1");
    const int64_t Ib = I;
    const size_t tb = dev ? (size_t)FR_HEAD * 8 : fr_host_table_bytes(tables, T, F);
    const int64_t ntiles = (j1 - j0 + FR_TJ - 1) / FR_TJ;
    if (B * ntiles > 0x7fffffffLL) return fail(ctx, GRIDHIP_EUNSUPPORTED, "fringe_search: more than 2^31 - 1 delay tiles");
    const size_t n = (size_t)B * T * F, pb = (size_t)B * I * FR_ROW * 8, sb = (size_t)I * A * 32, ib = (size_t)B * 8;
    if (outputs_clash({{peaks, pb}, {stats, 64}},
                      {{tables, tb}, {vis, n * 16}, {model_vis, n * 16}, {wt, n * 8}, {a1, ib}, {a2, ib}, {sol, sb}}))
        return fail(ctx, GRIDHIP_EINVAL, "fringe_search: arrays overlap");
    GH_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    DevBuf cnt, cand;
    GH_CHECK(cnt.alloc(ctx, sizeof(FrCount)));
    GH_CHECK(cand.alloc(ctx, (size_t)B * Ib * ntiles * 32));
    Staged sg(ctx, dev);
    FrSearch a{};
    a.B = (int)B, a.T = (int)T, a.F = (int)F, a.A = (int)A;
    a.tables = sg.in(tables, tb);
    a.vis = reinterpret_cast<const double2 *>(sg.in(vis, n * 16));
    a.model = reinterpret_cast<const double2 *>(sg.in(model_vis, n * 16));
    a.wt = sg.in(wt, n * 8), a.a1 = sg.in(a1, ib), a.a2 = sg.in(a2, ib), a.sol = sg.in(sol, sb);
    a.peaks = sg.inout(peaks, peaks, pb);  // (a table that does not fit leaves them as they are, in the host form too)
    stats = sg.out(stats, 64);
    a.mode = 0, a.j0 = (int)j0, a.j1 = (int)j1, a.k0 = (int)k0, a.k1 = (int)k1;
    a.ntiles = (int)ntiles, a.Ib = (int)Ib, a.cand = cand.as<double>(), a.cnt = cnt.as<FrCount>();
    GH_CHECK(sg.status());
    fr_search_launch(ctx, a, Ib, stats);
    GH_CHECK_HIP(ctx, hipGetLastError());
    return sg.finish();
}

bool fr_solve_args_ok(int64_t B, int64_t I, int64_t A, double min_count, double min_coh2, int64_t refant, int64_t niter,
                      double tol)
{
    return B >= 1 && I >= 1 && A >= 2 && min_count >= 0.0 && isfinite(min_count) && min_coh2 >= 0.0 && isfinite(min_coh2) &&
           refant < A && niter >= 0 && niter <= GRIDHIP_FRINGE_MAX_ITER && tol >= 0.0 && isfinite(tol);
}

int fr_solve_any(gridhip_ctx *ctx, bool dev, int64_t B, int64_t I, int64_t A, const int64_t *a1, const int64_t *a2,
                 const double *peaks, double min_count, double min_coh2, int64_t refant, int64_t niter, double tol,
                 double *sol, double *info, double *stats)
{
    if (!ctx) return GRIDHIP_EINVAL;
    if (!fr_solve_args_ok(B, I, A, min_count, min_coh2, refant, niter, tol) || !a1 || !a2 || !peaks || !sol || !info || !stats)
        return fail(ctx, GRIDHIP_EINVAL, "fringe_solve: bad argument");
    if (!fr_cube_fits(B, I, A)) return fail(ctx, GRIDHIP_EUNSUPPORTED, "fringe_solve: B above 2^24, I above 2^20 or A above 1024");
    const size_t pb = (size_t)B * I * FR_ROW * 8, sb = (size_t)I * A * 32, nb = (size_t)I * A * 8, ib = (size_t)B * 8;
    if (outputs_clash({{sol, sb}, {info, nb}, {stats, 64}}, {{a1, ib}, {a2, ib}, {peaks, pb}}))
        return fail(ctx, GRIDHIP_EINVAL, "fringe_solve: arrays overlap");
    GH_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    DevBuf w, part, edges;
    GH_CHECK(w.alloc(ctx, (size_t)I * B * 8));
    GH_CHECK(part.alloc(ctx, (size_t)I * 64));
    GH_CHECK(edges.alloc(ctx, (size_t)I * B * 2 * sizeof(FrEdge)));
    Staged sg(ctx, dev);
    FrSolve a{};
    a.B = (int)B, a.I = (int)I, a.A = (int)A;
    a.a1 = sg.in(a1, ib), a.a2 = sg.in(a2, ib), a.peaks = sg.in(peaks, pb);
    a.min_count = min_count, a.min_coh2 = min_coh2, a.refant = (int)(refant < 0 ? -1 : refant), a.niter = (int)niter, a.tol = tol;
    a.sol = sg.inout(sol, sol, sb), a.info = sg.out(info, nb);
    stats = sg.out(stats, 64);
    a.w = w.as<double>(), a.part = part.as<double>(), a.edges = edges.as<FrEdge>();
    GH_CHECK(sg.status());
    fr_solve_launch(ctx, a, stats);
    GH_CHECK_HIP(ctx, hipGetLastError());
    return sg.finish();
}

int fr_fit_any(gridhip_ctx *ctx, bool dev, int64_t B, int64_t T, int64_t F, int64_t A, int64_t I, int64_t Nd, int64_t Nr,
               const double *tables, const double *vis, const double *model_vis, const double *wt, const int64_t *a1,
               const int64_t *a2, int64_t rounds, int64_t wj, int64_t wk, double min_count, double min_coh2, int64_t refant,
               int64_t niter, double tol, int warm, double *sol, double *peaks, double *info, double *stats)
{
    if (!ctx) return GRIDHIP_EINVAL;
    if (!fr_cube_ok(B, T, F, A) || I < 1 || I > T || Nd < 1 || Nd > FR_MAX_ND || Nr < 1 || Nr > FR_MAX_NR || !tables || !vis ||
        !a1 || !a2 || !sol || !peaks || !info || !stats || rounds < 1 || rounds > GRIDHIP_FRINGE_MAX_ROUNDS || wj < 0 ||
        wj > FR_MAX_ND || wk < 0 || wk > FR_MAX_NR || (warm != 0 && warm != 1) ||
        !fr_solve_args_ok(B, I, A, min_count, min_coh2, refant, niter, tol) || ((uintptr_t)vis & 15) ||
        ((uintptr_t)model_vis & 15))
        return fail(ctx, GRIDHIP_EINVAL, "fringefit: bad argument");
    const int64_t ntiles0 = (Nd + FR_TJ - 1) / FR_TJ, ntiles1 = (2 * wj + 1 + FR_TJ - 1) / FR_TJ;
    const int64_t ntmax = ntiles0 > ntiles1 ? ntiles0 : ntiles1;
    if (!fr_cube_fits(B, T, A) || B * T > ((int64_t)1 << 31) - 1 || B * ntmax > 0x7fffffffLL)
        return fail(ctx, GRIDHIP_EUNSUPPORTED, "fringefit: B above 2^24, T above 2^20, A above 1024, or too many tiles");
    const size_t n = (size_t)B * T * F, tb = fr_table_bytes(F, T, Nd, Nr), pb = (size_t)B * I * FR_ROW * 8;
    const size_t sb = (size_t)I * A * 32, nb = (size_t)I * A * 8, ib = (size_t)B * 8;
    if (outputs_clash({{sol, sb}, {peaks, pb}, {info, nb}, {stats, 64}},
                      {{tables, tb}, {vis, n * 16}, {model_vis, n * 16}, {wt, n * 8}, {a1, ib}, {a2, ib}}))
        return fail(ctx, GRIDHIP_EINVAL, "fringefit: arrays overlap");
    GH_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    DevBuf cnt, cand, w, part, st, edges;
    GH_CHECK(cnt.alloc(ctx, sizeof(FrCount)));
    GH_CHECK(cand.alloc(ctx, (size_t)B * I * ntmax * 32));
    GH_CHECK(w.alloc(ctx, (size_t)I * B * 8));
    GH_CHECK(part.alloc(ctx, (size_t)I * 64));
    GH_CHECK(st.alloc(ctx, 128));
    GH_CHECK(edges.alloc(ctx, (size_t)I * B * 2 * sizeof(FrEdge)));
    Staged sg(ctx, dev);
    FrSearch a{};
    a.B = (int)B, a.T = (int)T, a.F = (int)F, a.A = (int)A;
    a.tables = sg.in(tables, tb);
    a.vis = reinterpret_cast<const double2 *>(sg.in(vis, n * 16));
    a.model = reinterpret_cast<const double2 *>(sg.in(model_vis, n * 16));
    a.wt = sg.in(wt, n * 8), a.a1 = sg.in(a1, ib), a.a2 = sg.in(a2, ib);
    double *dsol = sg.inout(sol, sol, sb);
    a.peaks = sg.inout(peaks, peaks, pb);
    double *dinfo = sg.inout(info, info, nb);
    stats = sg.out(stats, 64);
    a.Ib = (int)I, a.cand = cand.as<double>(), a.cnt = cnt.as<FrCount>();
    GH_CHECK(sg.status());
    FrSolve v{};
    v.B = (int)B, v.I = (int)I, v.A = (int)A, v.a1 = a.a1, v.a2 = a.a2, v.peaks = a.peaks;
    v.min_count = min_count, v.min_coh2 = min_coh2, v.refant = (int)(refant < 0 ? -1 : refant), v.niter = (int)niter, v.tol = tol;
    v.sol = dsol, v.info = dinfo, v.w = w.as<double>(), v.part = part.as<double>(), v.edges = edges.as<FrEdge>();
    double *ss = st.as<double>(), *vs = ss + 8;
    v.gate = ss;
    if (!warm)
        hipLaunchKernelGGL(fr_init_sol_kernel, dim3((unsigned)((I * A + 255) / 256)), dim3(256), 0, ctx->stream, I * A, dsol);
    for (int64_t r = 0; r < rounds; ++r) {
        if (r == 0) {
            a.mode = 2, a.j0 = 0, a.j1 = (int)Nd, a.k0 = 0, a.k1 = (int)Nr, a.ntiles = (int)ntiles0;
            a.sol = warm ? dsol : nullptr;
        } else {
            a.mode = 1, a.wj = (int)wj, a.wk = (int)wk, a.ntiles = (int)ntiles1, a.sol = dsol;
        }
        fr_search_launch(ctx, a, I, ss);
        fr_solve_launch(ctx, v, vs);
    }
    hipLaunchKernelGGL(fr_fit_stats_kernel, dim3(1), dim3(64), 0, ctx->stream, (int)T, (int)F, (int)I, a.tables,
                       (const double *)ss, (const double *)vs, stats);
    GH_CHECK_HIP(ctx, hipGetLastError());
    return sg.finish();
}

int fr_apply_any(gridhip_ctx *ctx, bool dev, int64_t B, int64_t T, int64_t F, int64_t A, int64_t I, const double *tables,
                 const double *sol, const int64_t *a1, const int64_t *a2, int inverse, const double *vis_in,
                 const double *wt_in, double *vis_out, double *wt_out)
{
    if (!ctx) return GRIDHIP_EINVAL;
    if (!fr_cube_ok(B, T, F, A) || I < 1 || I > T || !tables || !sol || !a1 || !a2 || !vis_in || !vis_out || (inverse != 0 && inverse != 1) ||
        ((uintptr_t)vis_in & 15) || ((uintptr_t)vis_out & 15))
        return fail(ctx, GRIDHIP_EINVAL, "apply_fringe: bad argument");
    if (!fr_cube_fits(B, T, A)) return fail(ctx, GRIDHIP_EUNSUPPORTED, "apply_fringe: B above 2^24, T above 2^20 or A above 1024");
    const size_t tb = dev ? (size_t)FR_HEAD * 8 : fr_host_table_bytes(tables, T, F);
    const size_t n = (size_t)B * T * F, sb = (size_t)I * A * 32, ib = (size_t)B * 8;
    if (outputs_clash({{vis_out, n * 16}, {wt_out, n * 8}},
                      {{vis_in, n * 16}, {wt_in, n * 8}, {tables, tb}, {sol, sb}, {a1, ib}, {a2, ib}}, {{0, 0}, {1, 1}}))
        return fail(ctx, GRIDHIP_EINVAL, "apply_fringe: arrays overlap");
    GH_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    Staged sg(ctx, dev);
    FrApply a{};
    a.B = (int)B, a.T = (int)T, a.F = (int)F, a.A = (int)A, a.I = (int)I, a.inverse = inverse;
    a.tables = sg.in(tables, tb), a.sol = sg.in(sol, sb), a.a1 = sg.in(a1, ib), a.a2 = sg.in(a2, ib);
    // a table that does not fit leaves the outputs as they are, in the host form too: an output's block starts from the
    // output's own bytes, and is the input's block only in place
    a.vis_out = reinterpret_cast<double2 *>(sg.inout(vis_out, vis_out, n * 16));
    a.vis_in = vis_in == vis_out ? a.vis_out : reinterpret_cast<const double2 *>(sg.in(vis_in, n * 16));
    a.wt_out = sg.inout(wt_out, wt_out, n * 8);
    a.wt_in = !wt_out ? nullptr : wt_in == wt_out ? a.wt_out : sg.in(wt_in, n * 8);  // (read only for wt_out)
    GH_CHECK(sg.status());
    hipLaunchKernelGGL(fr_apply_kernel, grid_for(ctx, (int64_t)n), dim3(256), 0, ctx->stream, a);
    GH_CHECK_HIP(ctx, hipGetLastError());
    return sg.finish();
}

}  // namespace

// what fringe_solve.h declares: the solve as another driver (tec.hip) enqueues it
bool fringe_solve_args_ok(int64_t B, int64_t I, int64_t A, double min_count, double min_coh2, int64_t refant, int64_t niter,
                          double tol)
{
    return fr_solve_args_ok(B, I, A, min_count, min_coh2, refant, niter, tol);
}

void fringe_solve_enqueue(gridhip_ctx *ctx, const FrSolve &a, double *stats) { fr_solve_launch(ctx, a, stats); }

void fringe_init_sol_enqueue(gridhip_ctx *ctx, int64_t n, double *sol)
{
    hipLaunchKernelGGL(fr_init_sol_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, n, sol);
}

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

int gridhip_fringe_solve(gridhip_ctx *ctx, int64_t B, int64_t I, int64_t A, const int64_t *a1, const int64_t *a2,
                         const double *peaks, double min_count, double min_coh2, int64_t refant, int64_t niter, double tol,
                         double *sol, double *info, double *stats)
{
    return fr_solve_any(ctx, false, B, I, A, a1, a2, peaks, min_count, min_coh2, refant, niter, tol, sol, info, stats);
}

int gridhip_fringe_solve_dev(gridhip_ctx *ctx, int64_t B, int64_t I, int64_t A, const int64_t *a1, const int64_t *a2,
                             const double *peaks, double min_count, double min_coh2, int64_t refant, int64_t niter,
                             double tol, double *sol, double *info, double *stats)
{
    return fr_solve_any(ctx, true, B, I, A, a1, a2, peaks, min_count, min_coh2, refant, niter, tol, sol, info, stats);
}

int gridhip_fringefit(gridhip_ctx *ctx, int64_t B, int64_t T, int64_t F, int64_t A, int64_t I, int64_t Nd, int64_t Nr,
                      const double *tables, const double *vis, const double *model_vis, const double *wt, const int64_t *a1,
                      const int64_t *a2, int64_t rounds, int64_t wj, int64_t wk, double min_count, double min_coh2,
                      int64_t refant, int64_t niter, double tol, int warm, double *sol, double *peaks, double *info,
                      double *stats)
{
    return fr_fit_any(ctx, false, B, T, F, A, I, Nd, Nr, tables, vis, model_vis, wt, a1, a2, rounds, wj, wk, min_count,
                      min_coh2, refant, niter, tol, warm, sol, peaks, info, stats);
}

int gridhip_fringefit_dev(gridhip_ctx *ctx, int64_t B, int64_t T, int64_t F, int64_t A, int64_t I, int64_t Nd, int64_t Nr,
                          const double *tables, const double *vis, const double *model_vis, const double *wt,
                          const int64_t *a1, const int64_t *a2, int64_t rounds, int64_t wj, int64_t wk, double min_count,
                          double min_coh2, int64_t refant, int64_t niter, double tol, int warm, double *sol, double *peaks,
                          double *info, double *stats)
{
    return fr_fit_any(ctx, true, B, T, F, A, I, Nd, Nr, tables, vis, model_vis, wt, a1, a2, rounds, wj, wk, min_count,
                      min_coh2, refant, niter, tol, warm, sol, peaks, info, stats);
}

int gridhip_apply_fringe(gridhip_ctx *ctx, int64_t B, int64_t T, int64_t F, int64_t A, int64_t I, const double *tables,
                         const double *sol, const int64_t *a1, const int64_t *a2, int inverse, const double *vis_in,
                         const double *wt_in, double *vis_out, double *wt_out)
{
    return fr_apply_any(ctx, false, B, T, F, A, I, tables, sol, a1, a2, inverse, vis_in, wt_in, vis_out, wt_out);
}

int gridhip_apply_fringe_dev(gridhip_ctx *ctx, int64_t B, int64_t T, int64_t F, int64_t A, int64_t I, const double *tables,
                             const double *sol, const int64_t *a1, const int64_t *a2, int inverse, const double *vis_in,
                             const double *wt_in, double *vis_out, double *wt_out)
{
    return fr_apply_any(ctx, true, B, T, F, A, I, tables, sol, a1, a2, inverse, vis_in, wt_in, vis_out, wt_out);
}

int gridhip_fringe_tile(int64_t *out)
{
    if (!out) return GRIDHIP_EINVAL;
    out[0] = FR_TJ, out[1] = FR_KC, out[2] = FR_TR;
    return GRIDHIP_OK;
}

}  // extern "C"
