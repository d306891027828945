// Dispersive delay (TEC) calibration (include/gridhip.h, "dispersive delay (TEC) calibration"): a search per baseline and
// solution interval over a grid of delays and orthogonalised TEC cells, the antenna fit of fringe.hip, and the apply step.
//
//     gridhip_tec_tables   tc_head_kernel (one work-group: the checks, s, the head), tc_fill_kernel (one thread per entry)
//     gridhip_tec_search   tc_zero_kernel, tc_search_kernel, tc_refine_kernel, tc_search_stats_kernel
//     gridhip_tecfit       [the solve's init]; per round the four above and the two of the solve; tc_fit_stats_kernel
//     gridhip_apply_tec    tc_apply_kernel (one thread per sample)
// Every kernel that reads a table judges its head itself and leaves at once when it does not fit the call; nothing is
// read back, so every _dev form is a fixed chain of launches.
//
// THE SEARCH KERNEL.  A work-group of 256 threads owns one (baseline, interval) and a tile of TC_TJ = 512 delays x TC_TM = 8
// TEC cells.  It forms Xbar[f] = sum_t X'[t][f] once in LDS (16 KB): a thread owns the channels tid, tid + 256, ..., makes
// their derotation phasor once and walks the time steps in order, so that every row of samples is read coalesced along f.
// Ef and Em then pass through LDS in chunks of TC_KC = 4 channels (32 KB + 4 KB); a tile of fewer delays - a window round's
// five - stages rows as wide as it needs and up to 32 channels at a time, so that it waits for memory 8 times, not 64,
// across 256 channels.  A lane keeps the accumulators of TC_RJ = 2 delays (64 apart: a wave reads 64 consecutive Ef
// entries) and of the tile's TEC cells in registers: one product
// Em Xbar per (f, m) feeds both delays, and an Ef entry feeds every TEC cell of the tile.  The number of TEC cells a
// lane carries is the tile's own - 1, 2, 4 or 8, an instantiation each - so a grid of three TEC cells does not pay for
// eight.  Every accumulator adds its channels in ascending order, unfused; a running (P, j, m) maximum per lane is reduced
// by the tie rule (largest P, lowest j, lowest m) into one candidate per tile.  52 KB of LDS: three work-groups share a CU.
// No matrix instruction (v_mfma_f64 fixes its own order and fuses).
// THE REFINEMENT KERNEL.  One wave per (baseline, interval) takes the best candidate over the tiles, forms Xbar again
// by the same device function, recomputes S at the peak and its four neighbours by the same ordered sum - so the bits do
// not depend on the tile borders - and forms the energy, the counts and the row of `peaks`.
#include "common.h"
#include "fringe_solve.h"
#include "imaging.h"

#pragma clang fp contract(off)

namespace gridhip {

namespace {

typedef unsigned long long u64;

constexpr int TC_THREADS = 256;
constexpr int TC_RJ = 2;                                  // delays of a lane
constexpr int TC_TJ = TC_THREADS * TC_RJ;                 // delays of a work-group
constexpr int TC_TM = 8;                                  // TEC cells of a work-group
constexpr int TC_KC = 4;                                  // channels of a staged chunk of a full tile
constexpr int TC_ES = TC_KC * TC_TJ;                      // the Ef entries staged at a time
constexpr int TC_KMAX = TC_ES / 64;                       // channels of a staged chunk of the narrowest tile
constexpr int TC_HEAD = GRIDHIP_TEC_HEAD, TC_ROW = GRIDHIP_TEC_PEAK;
constexpr int TC_MAX_F = GRIDHIP_TEC_MAX_CHANNELS, TC_MAX_ND = GRIDHIP_TEC_MAX_DELAYS, TC_MAX_NM = GRIDHIP_TEC_MAX_CELLS;
constexpr int TC_MAX_A = GRIDHIP_FRINGE_MAX_ANTENNAS;

struct TcCount {  // the counters of one search
    u64 flagged, bad, empty, refused, ok;
    u64 pad[3];
};

struct TcHead {
    bool ok;
    int F, T, tint, I, Nd, Nm;
    double tau0, dtau, tec0, dtec;
    const double2 *Ef, *Em;
    const double *af, *cf;
};

__device__ __forceinline__ bool tc_finite(double x) { return __builtin_isfinite(x); }

__device__ __forceinline__ bool tc_int_in(double v, int lo, int hi) { return v >= (double)lo && v <= (double)hi && v == (double)(int)v; }

// the head of a table, and whether it fits a cube of T time steps and F channels
__device__ __forceinline__ TcHead tc_head(const double *tb, int T, int F)
{
    TcHead h;
    h.ok = tb[0] == 1.0 && tb[1] == (double)F && tb[2] == (double)T && T >= 1 && tc_int_in(tb[3], 1, T) &&
           tc_int_in(tb[5], 1, TC_MAX_ND) && tc_int_in(tb[6], 1, TC_MAX_NM) && F >= 1 && F <= TC_MAX_F;
    h.F = F, h.T = T;
    h.tint = h.ok ? (int)tb[3] : 1, h.Nd = h.ok ? (int)tb[5] : 1, h.Nm = h.ok ? (int)tb[6] : 1;
    h.I = (T + h.tint - 1) / h.tint;
    h.ok = h.ok && tb[4] == (double)h.I;
    h.tau0 = tb[7], h.dtau = tb[8], h.tec0 = tb[9], h.dtec = tb[10];
    const double *p = tb + TC_HEAD;
    h.Ef = reinterpret_cast<const double2 *>(p), p += 2 * (int64_t)F * h.Nd;
    h.Em = reinterpret_cast<const double2 *>(p), p += 2 * (int64_t)F * h.Nm;
    h.af = p, h.cf = p + F;
    return h;
}

// the fringe section's phasor recipe and products
__device__ __forceinline__ double2 tc_phasor(double a, double b)
{
    const double x = a * b;
    const double r = x - rint(x);
    double sn, cs;
    sincospi(2.0 * r, &sn, &cs);
    return make_double2(cs, sn);
}

__device__ __forceinline__ double2 tc_mulc(double2 x, double2 c) { return make_double2(x.x * c.x + x.y * c.y, x.y * c.x - x.x * c.y); }
__device__ __forceinline__ double2 tc_mul(double2 x, double2 c) { return make_double2(x.x * c.x - x.y * c.y, x.x * c.y + x.y * c.x); }
__device__ __forceinline__ void tc_mac(double2 &acc, double2 e, double2 x)
{
    acc.x = acc.x + (e.x * x.x - e.y * x.y);
    acc.y = acc.y + (e.x * x.y + e.y * x.x);
}

// z_f = -(kappa (1 / nu_f - 1 / nu0)), every operation rounded
__device__ __forceinline__ double tc_z(double nu, double nu0) { return -(GRIDHIP_TEC_KAPPA * (1.0 / nu - 1.0 / nu0)); }

__global__ void __launch_bounds__(256)
    tc_head_kernel(int F, int T, int tint, int Nd, int Nm, const double *__restrict__ freq, double tau0, double dtau,
                   double tec0, double dtec, double *__restrict__ tables)
{
    if (blockIdx.x != 0) return;
    int bad = 0;  // the one work-group shares the scan of freq
    for (int i = threadIdx.x; i < F; i += blockDim.x) bad |= !(tc_finite(freq[i]) && freq[i] > 0.0);
    bad = __syncthreads_or(bad);
    if (threadIdx.x != 0) return;
    const double nu0 = freq[0] + 0.5 * (freq[F - 1] - freq[0]);
    double s = 0.0;
    if (!bad) {
        double num = 0.0, den = 0.0;
        for (int f = 0; f < F; ++f) {
            const double a = freq[f] - nu0, z = tc_z(freq[f], nu0);
            num = num + a * z, den = den + a * a;
        }
        s = den > 0.0 ? num / den : 0.0;
    }
    const bool ok = !bad && tc_finite(tau0) && tc_finite(dtau) && tc_finite(tec0) && tc_finite(dtec) && dtau > 0.0 &&
                    dtec > 0.0 && tc_finite(nu0) && tc_finite(s);
    for (int i = 0; i < TC_HEAD; ++i) tables[i] = 0.0;
    tables[0] = ok ? 1.0 : 0.0;
    tables[1] = (double)F, tables[2] = (double)T, tables[3] = (double)tint, tables[4] = (double)((T + tint - 1) / tint);
    tables[5] = (double)Nd, tables[6] = (double)Nm, tables[7] = tau0, tables[8] = dtau, tables[9] = tec0, tables[10] = dtec;
    tables[11] = ok ? nu0 : 0.0, tables[12] = ok ? s : 0.0, tables[13] = GRIDHIP_TEC_KAPPA;
}

__global__ void __launch_bounds__(256) tc_fill_kernel(int F, int Nd, int Nm, const double *__restrict__ freq, double *tables)
{
    const bool valid = tables[0] == 1.0;
    const double tau0 = tables[7], dtau = tables[8], tec0 = tables[9], dtec = tables[10], nu0 = tables[11], s = tables[12];
    const int64_t nF = (int64_t)F * Nd, nM = (int64_t)F * Nm, total = nF + nM + 2 * (int64_t)F;
    double *Ef = tables + TC_HEAD, *Em = Ef + 2 * nF, *af = Em + 2 * nM, *cf = af + F;
    const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, step = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = i0; i < total; i += step) {
        if (i < nF) {
            double2 e = make_double2(0.0, 0.0);
            if (valid) {
                const int f = (int)(i / Nd), j = (int)(i % Nd);
                e = tc_phasor(tau0 + (double)j * dtau, freq[f] - nu0);
            }
            Ef[2 * i] = e.x, Ef[2 * i + 1] = -e.y;
        } else if (i < nF + nM) {
            const int64_t k = i - nF;
            double2 e = make_double2(0.0, 0.0);
            if (valid) {
                const int f = (int)(k / Nm), m = (int)(k % Nm);
                const double a = freq[f] - nu0;
                e = tc_phasor(tec0 + (double)m * dtec, tc_z(freq[f], nu0) - s * a);
            }
            Em[2 * k] = e.x, Em[2 * k + 1] = -e.y;
        } else if (i < nF + nM + F) {
            const int f = (int)(i - nF - nM);
            af[f] = valid ? freq[f] - nu0 : 0.0;
        } else {
            const int f = (int)(i - nF - nM - F);
            double v = 0.0;
            if (valid) {
                const double a = freq[f] - nu0;
                v = tc_z(freq[f], nu0) - s * a;
            }
            cf[f] = v;
        }
    }
}

struct TcSearch {
    int B, T, F, A;
    const double *tables;
    const double2 *vis, *model;
    const double *wt;
    const int64_t *a1, *a2;
    const double *sol;
    int mode;  // 0: the cells [j0, j1) x [m0, m1); 1: those within (wj, wm) of the grid's zero; 2: the whole grid, j1 = Nd, m1 = Nm
    int j0, j1, m0, m1, wj, wm;
    int ntj, ntm, Ib;  // the tiles launched along either axis, and the caller's I: the table's, or the call does not fit
    double *cand;      // [B][Ib][ntj * ntm][4] = { P, j, m, 0 }, P = -1: none
    double *peaks;
    TcCount *cnt;
};

// the cells of a search; false: the call does not fit the table
__device__ __forceinline__ bool tc_window(const TcHead &h, const TcSearch &a, int *j0, int *j1, int *m0, int *m1)
{
    if (!h.ok || h.I != a.Ib) return false;
    if (a.mode == 1) {
        double zj = rint(-h.tau0 / h.dtau), zm = rint(-h.tec0 / h.dtec);
        zj = zj > 0.0 ? zj : 0.0, zm = zm > 0.0 ? zm : 0.0;  // (a NaN goes to 0)
        const int cj = zj < (double)(h.Nd - 1) ? (int)zj : h.Nd - 1, cm = zm < (double)(h.Nm - 1) ? (int)zm : h.Nm - 1;
        *j0 = cj - a.wj > 0 ? cj - a.wj : 0, *j1 = cj + a.wj + 1 < h.Nd ? cj + a.wj + 1 : h.Nd;
        *m0 = cm - a.wm > 0 ? cm - a.wm : 0, *m1 = cm + a.wm + 1 < h.Nm ? cm + a.wm + 1 : h.Nm;
    } else {
        *j0 = a.j0, *j1 = a.j1, *m0 = a.m0, *m1 = a.m1;
        if (a.mode == 2 && (a.j1 != h.Nd || a.m1 != h.Nm)) return false;
    }
    return *j0 >= 0 && *j0 < *j1 && *j1 <= h.Nd && *m0 >= 0 && *m0 < *m1 && *m1 <= h.Nm &&
           (*j1 - *j0 + TC_TJ - 1) / TC_TJ <= a.ntj && (*m1 - *m0 + TC_TM - 1) / TC_TM <= a.ntm;
}

struct TcDerot {  // the derotation of one (baseline, interval)
    bool on;
    double2 d;
    double dtau, dtec;
};

__device__ __forceinline__ TcDerot tc_derotation(const TcSearch &a, int i, int p, int q)
{
    TcDerot r;
    r.on = a.sol != nullptr, r.d = make_double2(1.0, 0.0), r.dtau = 0.0, r.dtec = 0.0;
    if (r.on) {
        const double *sp = a.sol + ((int64_t)i * a.A + p) * 4, *sq = a.sol + ((int64_t)i * a.A + q) * 4;
        r.dtau = sp[0] - sq[0], r.dtec = sp[1] - sq[1];
        r.d = tc_mulc(make_double2(sp[2], sp[3]), make_double2(sq[2], sq[3]));
    }
    return r;
}

// Dfm[f] = ph(tau_p - tau_q, a_f) ph(tec_p - tec_q, c_f)
__device__ __forceinline__ double2 tc_dfm(const TcHead &h, const TcDerot &r, int f)
{
    return tc_mul(tc_phasor(r.dtau, h.af[f]), tc_phasor(r.dtec, h.cf[f]));
}

// X' of the sample at `at`; *flagged: its weight is not > 0 and it is (0, 0)
__device__ __forceinline__ double2 tc_sample(const TcSearch &a, int64_t at, const TcDerot &r, double2 dfm, bool *flagged)
{
    const double s = a.wt ? a.wt[at] : 1.0;
    *flagged = !(s > 0.0);
    if (*flagged) return make_double2(0.0, 0.0);
    const double2 v = a.vis[at];
    double2 x = make_double2(s * v.x, s * v.y);
    if (a.model) x = tc_mulc(x, a.model[at]);
    if (r.on) x = tc_mulc(tc_mulc(x, r.d), dfm);
    return x;
}

// Xbar[f] = sum_t X'[t][f] into LDS, t ascending from (0, 0); a thread owns the channels tid, tid + nthreads, ...
__device__ __forceinline__ void tc_xbar(const TcSearch &a, const TcHead &h, const TcDerot &r, int b, int t0, int nt, double2 *Xs,
                                        int tid, int nthreads)
{
    for (int f = tid; f < h.F; f += nthreads) {
        const double2 dfm = r.on ? tc_dfm(h, r, f) : make_double2(1.0, 0.0);
        double2 acc = make_double2(0.0, 0.0);
        for (int t = 0; t < nt; ++t) {
            bool fl;
            const double2 x = tc_sample(a, ((int64_t)b * h.T + t0 + t) * h.F + f, r, dfm, &fl);
            acc.x = acc.x + x.x, acc.y = acc.y + x.y;
        }
        Xs[f] = acc;
    }
}

// is (q, qj, qm) ahead of (p, pj, pm)?  The largest power, then the lowest delay, then the lowest TEC cell; a "none"
// (-1, -1, -1) is behind everything, and a NaN is ahead of nothing
__device__ __forceinline__ bool tc_ahead(double q, int qj, int qm, double p, int pj, int pm)
{
    return q > p || (q == p && (qj < pj || (qj == pj && qm < pm)));
}

__global__ void tc_zero_kernel(TcCount *cnt)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) *cnt = TcCount{};
}

// the tile's sums with RM TEC cells per lane, and the lane's best cell
template <int RM>
__device__ __forceinline__ void tc_tile(const TcHead &h, const double2 *Xs, double2 *Es, double2 *Ms, int jt0, int j1, int mt0,
                                        int m1, int tid, double *bp, int *bj, int *bm)
{
    const int lane = tid & 63, wv = tid >> 6;
    const int jl = wv * (64 * TC_RJ) + lane;  // the lane's delays within the tile: jl and jl + 64
    // a tile of nj delays stages rows of `stride` entries (nj rounded up to the 64 a wave reads) and as many channels as
    // then fit: TC_KC of a full tile, up to TC_KMAX of a window round's few delays, whose chunks would else be all waiting
    const int nj = j1 - jt0 < TC_TJ ? j1 - jt0 : TC_TJ;
    const int stride = (nj + 63) & ~63, kcap = TC_ES / stride;
    bool on[TC_RJ];
#pragma unroll
    for (int r = 0; r < TC_RJ; ++r) on[r] = jl + r * 64 < nj;
    double2 acc[TC_RJ][RM];
#pragma unroll
    for (int r = 0; r < TC_RJ; ++r)
#pragma unroll
        for (int mm = 0; mm < RM; ++mm) acc[r][mm] = make_double2(0.0, 0.0);
    for (int c0 = 0; c0 < h.F; c0 += kcap) {
        const int nk = h.F - c0 < kcap ? h.F - c0 : kcap;
        __syncthreads();  // (Xs is there; the chunk before has been read)
        for (int idx = tid; idx < nk * stride; idx += TC_THREADS) {
            const int kc = idx / stride, jj = idx % stride;
            Es[idx] = jj < nj ? h.Ef[(int64_t)(c0 + kc) * h.Nd + jt0 + jj] : make_double2(0.0, 0.0);
        }
        for (int idx = tid; idx < nk * TC_TM; idx += TC_THREADS) {
            const int kc = idx / TC_TM, mm = idx % TC_TM;
            Ms[idx] = mt0 + mm < m1 ? h.Em[(int64_t)(c0 + kc) * h.Nm + mt0 + mm] : make_double2(0.0, 0.0);
        }
        __syncthreads();
        if (on[0]) {  // (on[r] implies on[0])
            for (int kc = 0; kc < nk; ++kc) {
                const double2 x = Xs[c0 + kc];
                double2 pr[RM];
#pragma unroll
                for (int mm = 0; mm < RM; ++mm) pr[mm] = tc_mul(Ms[kc * TC_TM + mm], x);
#pragma unroll
                for (int r = 0; r < TC_RJ; ++r) {
                    if (!on[r]) continue;
                    const double2 e = Es[kc * stride + jl + r * 64];
#pragma unroll
                    for (int mm = 0; mm < RM; ++mm) tc_mac(acc[r][mm], e, pr[mm]);
                }
            }
        }
    }
#pragma unroll
    for (int r = 0; r < TC_RJ; ++r) {
        const int j = jt0 + jl + r * 64;
#pragma unroll
        for (int mm = 0; mm < RM; ++mm) {
            const int m = mt0 + mm;
            const double P = acc[r][mm].x * acc[r][mm].x + acc[r][mm].y * acc[r][mm].y;
            if (j < j1 && m < m1 && tc_ahead(P, j, m, *bp, *bj, *bm)) *bp = P, *bj = j, *bm = m;
        }
    }
}

__global__ void __launch_bounds__(TC_THREADS) tc_search_kernel(TcSearch a)
{
    __shared__ double2 Xs[TC_MAX_F];
    __shared__ double2 Es[TC_ES];
    __shared__ double2 Ms[TC_KMAX * TC_TM];
    __shared__ double rp[TC_THREADS / 64];
    __shared__ int rj[TC_THREADS / 64], rm[TC_THREADS / 64];
    const TcHead h = tc_head(a.tables, a.T, a.F);
    int j0, j1, m0, m1;
    if (!tc_window(h, a, &j0, &j1, &m0, &m1)) return;
    const int tid = threadIdx.x;
    const unsigned ntl = (unsigned)(a.ntj * a.ntm);
    const int tile = (int)(blockIdx.x % ntl);
    const unsigned bi = blockIdx.x / ntl;
    const int b = (int)(bi / (unsigned)h.I), i = (int)(bi % (unsigned)h.I);
    if (b >= a.B) return;
    const int jt0 = j0 + (tile / a.ntm) * TC_TJ, mt0 = m0 + (tile % a.ntm) * TC_TM;
    const int64_t p = a.a1[b], q = a.a2[b];
    double *c = a.cand + (((int64_t)b * a.Ib + i) * ntl + tile) * 4;
    const bool live = jt0 < j1 && mt0 < m1 && p >= 0 && p < a.A && q >= 0 && q < a.A && p != q;
    if (!live) {  // (the same for every thread)
        if (tid == 0) c[0] = -1.0, c[1] = -1.0, c[2] = -1.0, c[3] = 0.0;
        return;
    }
    const int t0 = i * h.tint, nt = h.T - t0 < h.tint ? h.T - t0 : h.tint;
    const TcDerot r = tc_derotation(a, i, (int)p, (int)q);
    tc_xbar(a, h, r, b, t0, nt, Xs, tid, TC_THREADS);
    double bp = -1.0;
    int bj = -1, bm = -1;
    const int nm = m1 - mt0;  // (the same for every thread)
    if (nm == 1)
        tc_tile<1>(h, Xs, Es, Ms, jt0, j1, mt0, m1, tid, &bp, &bj, &bm);
    else if (nm == 2)
        tc_tile<2>(h, Xs, Es, Ms, jt0, j1, mt0, m1, tid, &bp, &bj, &bm);
    else if (nm <= 4)
        tc_tile<4>(h, Xs, Es, Ms, jt0, j1, mt0, m1, tid, &bp, &bj, &bm);
    else
        tc_tile<TC_TM>(h, Xs, Es, Ms, jt0, j1, mt0, m1, tid, &bp, &bj, &bm);
    for (int o = 32; o > 0; o >>= 1) {
        const double qp = __shfl_xor(bp, o);
        const int qj = __shfl_xor(bj, o), qm = __shfl_xor(bm, o);
        if (tc_ahead(qp, qj, qm, bp, bj, bm)) bp = qp, bj = qj, bm = qm;
    }
    if ((tid & 63) == 0) rp[tid >> 6] = bp, rj[tid >> 6] = bj, rm[tid >> 6] = bm;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < TC_THREADS / 64; ++w)
            if (tc_ahead(rp[w], rj[w], rm[w], bp, bj, bm)) bp = rp[w], bj = rj[w], bm = rm[w];
        c[0] = bp, c[1] = (double)bj, c[2] = (double)bm, c[3] = 0.0;
    }
}

// the second half of the parabola rule of gridhip_rmclean: the offset in cells from the three powers, 0 where it does not apply
__device__ __forceinline__ double tc_parabola(double pm, double ps, double pp)
{
    const double d = (pm - ps) + (pp - ps);
    return d < 0.0 ? (0.5 * (pm - pp)) / d : 0.0;
}

__global__ void __launch_bounds__(64) tc_refine_kernel(TcSearch a)
{
    __shared__ double2 Dfs[TC_MAX_F], Xs[TC_MAX_F];
    __shared__ double es[64];
    const TcHead h = tc_head(a.tables, a.T, a.F);
    int j0, j1, m0, m1;
    if (!tc_window(h, a, &j0, &j1, &m0, &m1)) return;
    const int lane = threadIdx.x;
    const int b = (int)(blockIdx.x / (unsigned)h.I), i = (int)(blockIdx.x % (unsigned)h.I);
    if (b >= a.B) return;
    double *row = a.peaks + ((int64_t)b * h.I + i) * TC_ROW;
    const int64_t p = a.a1[b], q = a.a2[b];
    int code = 0;
    double out[TC_ROW] = {-1.0, -1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    u64 nflag = 0;
    if (!(p >= 0 && p < a.A && q >= 0 && q < a.A && p != q)) {  // (the same for every lane, as every branch below)
        code = 3;
    } else {
        const int t0 = i * h.tint, nt = h.T - t0 < h.tint ? h.T - t0 : h.tint;
        const TcDerot r = tc_derotation(a, i, (int)p, (int)q);
        const double2 one = make_double2(1.0, 0.0);
        if (r.on)
            for (int f = lane; f < h.F; f += 64) Dfs[f] = tc_dfm(h, r, f);
        tc_xbar(a, h, r, b, t0, nt, Xs, lane, 64);
        __syncthreads();
        // the energy and the counts: a lane owns a time step of a pass of 64; the passes and their steps are added in order
        int nu = 0, nf = 0;
        bool bad = false;
        double N = 0.0;
        for (int tb = 0; tb < nt; tb += 64) {
            const int t = tb + lane;
            double e = 0.0;
            if (t < nt) {
                for (int f = 0; f < h.F; ++f) {
                    bool fl;
                    const double2 x = tc_sample(a, ((int64_t)b * h.T + t0 + t) * h.F + f, r, r.on ? Dfs[f] : one, &fl);
                    if (fl) {
                        ++nf;
                    } else {
                        ++nu;
                        bad = bad || !(tc_finite(x.x) && tc_finite(x.y));
                        e = e + (x.x * x.x + x.y * x.y);
                    }
                }
            }
            es[lane] = e;
            __syncthreads();
            const int n = nt - tb < 64 ? nt - tb : 64;
            for (int k = 0; k < n; ++k) N = N + es[k];
            __syncthreads();
        }
        for (int o = 32; o > 0; o >>= 1) nu += __shfl_xor(nu, o), nf += __shfl_xor(nf, o);
        bad = __any(bad);
        nflag = (u64)nf;
        // the best candidate over the tiles of the window
        double bp = -1.0;
        int bj = -1, bm = -1;
        const int utj = (j1 - j0 + TC_TJ - 1) / TC_TJ, utm = (m1 - m0 + TC_TM - 1) / TC_TM;
        const double *cb = a.cand + ((int64_t)b * a.Ib + i) * ((int64_t)a.ntj * a.ntm) * 4;
        for (int tj = 0; tj < utj; ++tj)
            for (int tm = 0; tm < utm; ++tm) {
                const double *c = cb + ((int64_t)tj * a.ntm + tm) * 4;
                const double cp = c[0];
                if (cp >= 0.0 && tc_ahead(cp, (int)c[1], (int)c[2], bp, bj, bm)) bp = cp, bj = (int)c[1], bm = (int)c[2];
            }
        out[8] = (double)nu;
        if (nu == 0) {
            code = 1;
        } else if (bad || bj < j0 || bj >= j1 || bm < m0 || bm >= m1) {
            code = 2;
        } else {
            const bool inj = bj > j0 && bj < j1 - 1, inm = bm > m0 && bm < m1 - 1;
            // lane 0: (j*, m*); 1, 2: j* -+ 1; 3, 4: m* -+ 1
            double2 S = make_double2(0.0, 0.0);
            const bool mine = lane == 0 || ((lane == 1 || lane == 2) && inj) || ((lane == 3 || lane == 4) && inm);
            if (mine) {
                const int j = lane == 1 ? bj - 1 : lane == 2 ? bj + 1 : bj, m = lane == 3 ? bm - 1 : lane == 4 ? bm + 1 : bm;
                for (int f = 0; f < h.F; ++f)
                    tc_mac(S, h.Ef[(int64_t)f * h.Nd + j], tc_mul(h.Em[(int64_t)f * h.Nm + m], Xs[f]));
            }
            const double P = S.x * S.x + S.y * S.y;
            const double ps = __shfl(P, 0), pjm = __shfl(P, 1), pjp = __shfl(P, 2), pmm = __shfl(P, 3), pmp = __shfl(P, 4);
            const double sre = __shfl(S.x, 0), sim = __shfl(S.y, 0);
            double tau = h.tau0 + (double)bj * h.dtau, tec = h.tec0 + (double)bm * h.dtec;
            if (inj) tau = tau + tc_parabola(pjm, ps, pjp) * h.dtau;
            if (inm) tec = tec + tc_parabola(pmm, ps, pmp) * h.dtec;
            out[0] = (double)bj, out[1] = (double)bm, out[2] = ps, out[3] = tau, out[4] = tec;
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
        for (int c = 0; c < TC_ROW; ++c) row[c] = out[c];
        if (nflag) atomicAdd(&a.cnt->flagged, nflag);
        atomicAdd(code == 0 ? &a.cnt->ok : code == 1 ? &a.cnt->empty : code == 2 ? &a.cnt->bad : &a.cnt->refused, (u64)1);
    }
}

__global__ void tc_search_stats_kernel(TcSearch a, double *__restrict__ stats)
{
    if (blockIdx.x != 0 || threadIdx.x != 0 || !stats) return;
    const TcHead h = tc_head(a.tables, a.T, a.F);
    int j0, j1, m0, m1;
    const bool ok = tc_window(h, a, &j0, &j1, &m0, &m1);
    for (int i = 0; i < GRIDHIP_TEC_STATS; ++i) stats[i] = 0.0;
    if (ok) {
        stats[0] = (double)a.cnt->flagged, stats[1] = (double)a.cnt->bad, stats[2] = (double)a.cnt->empty;
        stats[3] = (double)a.cnt->refused, stats[4] = (double)a.cnt->ok;
    } else {
        stats[7] = 1.0;
    }
}

// the driver's stats from those of its last search and solve
__global__ void tc_fit_stats_kernel(int T, int F, int I, int Nd, int Nm, const double *__restrict__ tables,
                                    const double *__restrict__ ss, const double *__restrict__ vs, double *__restrict__ stats)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const TcHead h = tc_head(tables, T, F);
    for (int i = 0; i < GRIDHIP_TEC_STATS; ++i) stats[i] = 0.0;
    if (!h.ok || h.I != I || h.Nd != Nd || h.Nm != Nm || ss[7] != 0.0) {
        stats[7] = 1.0;
        return;
    }
    stats[0] = vs[0], stats[1] = ss[0], stats[2] = ss[1], stats[3] = ss[2], stats[4] = vs[2];
    stats[5] = vs[4] / h.dtau, stats[6] = vs[5] / h.dtec;
}

struct TcApply {
    int B, T, F, A, I;
    const double *tables, *sol;
    const int64_t *a1, *a2;
    int inverse;
    const double2 *vis_in;
    const double *wt_in;
    double2 *vis_out;
    double *wt_out;
};

__global__ void __launch_bounds__(256) tc_apply_kernel(TcApply a)
{
    const TcHead h = tc_head(a.tables, a.T, a.F);
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
            ok = tc_finite(sp[0]) && tc_finite(sp[1]) && tc_finite(sp[2]) && tc_finite(sp[3]) && tc_finite(sq[0]) &&
                 tc_finite(sq[1]) && tc_finite(sq[2]) && tc_finite(sq[3]);
            if (ok) {
                const double2 d = tc_mulc(make_double2(sp[2], sp[3]), make_double2(sq[2], sq[3]));
                const double2 dfm = tc_mul(tc_phasor(sp[0] - sq[0], h.af[f]), tc_phasor(sp[1] - sq[1], h.cf[f]));
                v = a.inverse ? tc_mulc(tc_mulc(v, d), dfm) : tc_mul(tc_mul(v, d), dfm);
            }
        }
        a.vis_out[at] = v;
        if (a.wt_out) a.wt_out[at] = ok ? wv : 0.0;
    }
}

size_t tc_table_bytes(int64_t F, int64_t Nd, int64_t Nm) { return (size_t)GRIDHIP_TEC_TABLE_DOUBLES(F, Nd, Nm) * 8; }

bool tc_cube_ok(int64_t B, int64_t T, int64_t F, int64_t A) { return B >= 1 && T >= 1 && F >= 1 && F <= TC_MAX_F && A >= 2; }

// EUNSUPPORTED beyond these: the kernels index baselines and time steps with 32 bits
bool tc_cube_fits(int64_t B, int64_t T, int64_t A) { return B <= (1 << 24) && T <= (1 << 20) && A <= TC_MAX_A; }

int tc_tables_any(gridhip_ctx *ctx, bool dev, int64_t F, int64_t T, int64_t tint, const double *freq, double tau0, double dtau,
                  int64_t Nd, double tec0, double dtec, int64_t Nm, double *tables)
{
    if (!ctx) return GRIDHIP_EINVAL;
    if (tint == 0) tint = T;
    if (F < 1 || F > TC_MAX_F || T < 1 || tint < 1 || tint > T || Nd < 1 || Nd > TC_MAX_ND || Nm < 1 || Nm > TC_MAX_NM || !freq ||
        !tables)
        return fail(ctx, GRIDHIP_EINVAL, "tec_tables: bad argument");
    if (T > (1 << 20)) return fail(ctx, GRIDHIP_EUNSUPPORTED, "tec_tables: T above 2^20");
    const size_t fb = (size_t)F * 8, ab = tc_table_bytes(F, Nd, Nm);
    if (outputs_clash({{tables, ab}}, {{freq, fb}})) return fail(ctx, GRIDHIP_EINVAL, "tec_tables: arrays overlap");
    GH_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    Staged sg(ctx, dev);
    freq = sg.in(freq, fb), tables = sg.out(tables, ab);
    GH_CHECK(sg.status());
    hipLaunchKernelGGL(tc_head_kernel, dim3(1), dim3(256), 0, ctx->stream, (int)F, (int)T, (int)tint, (int)Nd, (int)Nm, freq,
                       tau0, dtau, tec0, dtec, tables);
    hipLaunchKernelGGL(tc_fill_kernel, grid_for(ctx, F * Nd + F * Nm + 2 * F), dim3(256), 0, ctx->stream, (int)F, (int)Nd,
                       (int)Nm, freq, tables);
    GH_CHECK_HIP(ctx, hipGetLastError());
    return sg.finish();
}

// the size of a host form's table, from its head in host memory: the whole table where the head fits the cube, else the
// head alone (the kernels see the same head and leave)
size_t tc_host_table_bytes(const double *tables, int64_t T, int64_t F)
{
    const double tint = tables[3], Nd = tables[5], Nm = tables[6];
    if (tables[0] == 1.0 && tables[1] == (double)F && tables[2] == (double)T && tint >= 1.0 && tint <= (double)T &&
        tint == (double)(int64_t)tint && Nd >= 1.0 && Nd <= TC_MAX_ND && Nd == (double)(int64_t)Nd && Nm >= 1.0 &&
        Nm <= TC_MAX_NM && Nm == (double)(int64_t)Nm)
        return tc_table_bytes(F, (int64_t)Nd, (int64_t)Nm);
    return (size_t)TC_HEAD * 8;
}

void tc_search_launch(gridhip_ctx *ctx, const TcSearch &a, int64_t nI, double *stats)
{
    hipLaunchKernelGGL(tc_zero_kernel, dim3(1), dim3(64), 0, ctx->stream, a.cnt);
    hipLaunchKernelGGL(tc_search_kernel, dim3((unsigned)((int64_t)a.B * nI * a.ntj * a.ntm)), dim3(TC_THREADS), 0, ctx->stream, a);
    hipLaunchKernelGGL(tc_refine_kernel, dim3((unsigned)((int64_t)a.B * nI)), dim3(64), 0, ctx->stream, a);
    hipLaunchKernelGGL(tc_search_stats_kernel, dim3(1), dim3(64), 0, ctx->stream, a, stats);
}

int64_t tc_tiles(int64_t n, int64_t tile) { return (n + tile - 1) / tile; }

int tc_search_any(gridhip_ctx *ctx, bool dev, int64_t B, int64_t T, int64_t F, int64_t A, int64_t I, const double *tables,
                  const double *vis, const double *model_vis, const double *wt, const int64_t *a1, const int64_t *a2,
                  const double *sol, int64_t j0, int64_t j1, int64_t m0, int64_t m1, double *peaks, double *stats)
{
    if (!ctx) return GRIDHIP_EINVAL;
    if (!tc_cube_ok(B, T, F, A) || I < 1 || I > T || !tables || !vis || !a1 || !a2 || !peaks || !stats || j0 < 0 || j0 >= j1 ||
        j1 > TC_MAX_ND || m0 < 0 || m0 >= m1 || m1 > TC_MAX_NM || ((uintptr_t)vis & 15) || ((uintptr_t)model_vis & 15))
        return fail(ctx, GRIDHIP_EINVAL, "tec_search: bad argument");
    if (!tc_cube_fits(B, T, A) || B * T > ((int64_t)1 << 31) - 1)
        return fail(ctx, GRIDHIP_EUNSUPPORTED, "tec_search: B above 2^24, T above 2^20, A above 1024 or B T above 2^31 - 1");
    const size_t tb = dev ? (size_t)TC_HEAD * 8 : tc_host_table_bytes(tables, T, F);
    const int64_t ntj = tc_tiles(j1 - j0, TC_TJ), ntm = tc_tiles(m1 - m0, TC_TM);
    if (B * I * ntj * ntm > 0x7fffffffLL) return fail(ctx, GRIDHIP_EUNSUPPORTED, "tec_search: more than 2^31 - 1 tiles");
    const size_t n = (size_t)B * T * F, pb = (size_t)B * I * TC_ROW * 8, sb = (size_t)I * A * 32, ib = (size_t)B * 8;
    if (outputs_clash({{peaks, pb}, {stats, 64}},
                      {{tables, tb}, {vis, n * 16}, {model_vis, n * 16}, {wt, n * 8}, {a1, ib}, {a2, ib}, {sol, sb}}))
        return fail(ctx, GRIDHIP_EINVAL, "tec_search: arrays overlap");
    GH_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    DevBuf cnt, cand;
    GH_CHECK(cnt.alloc(ctx, sizeof(TcCount)));
    GH_CHECK(cand.alloc(ctx, (size_t)B * I * ntj * ntm * 32));
    Staged sg(ctx, dev);
    TcSearch a{};
    a.B = (int)B, a.T = (int)T, a.F = (int)F, a.A = (int)A;
    a.tables = sg.in(tables, tb);
    a.vis = reinterpret_cast<const double2 *>(sg.in(vis, n * 16));
    a.model = reinterpret_cast<const double2 *>(sg.in(model_vis, n * 16));
    a.wt = sg.in(wt, n * 8), a.a1 = sg.in(a1, ib), a.a2 = sg.in(a2, ib), a.sol = sg.in(sol, sb);
    a.peaks = sg.inout(peaks, peaks, pb);  // (a table that does not fit leaves them as they are, in the host form too)
    stats = sg.out(stats, 64);
    a.mode = 0, a.j0 = (int)j0, a.j1 = (int)j1, a.m0 = (int)m0, a.m1 = (int)m1;
    a.ntj = (int)ntj, a.ntm = (int)ntm, a.Ib = (int)I, a.cand = cand.as<double>(), a.cnt = cnt.as<TcCount>();
    GH_CHECK(sg.status());
    tc_search_launch(ctx, a, I, stats);
    GH_CHECK_HIP(ctx, hipGetLastError());
    return sg.finish();
}

int tc_fit_any(gridhip_ctx *ctx, bool dev, int64_t B, int64_t T, int64_t F, int64_t A, int64_t I, int64_t Nd, int64_t Nm,
               const double *tables, const double *vis, const double *model_vis, const double *wt, const int64_t *a1,
               const int64_t *a2, int64_t rounds, int64_t wj, int64_t wm, double min_count, double min_coh2, int64_t refant,
               int64_t niter, double tol, int warm, double *sol, double *peaks, double *info, double *stats)
{
    if (!ctx) return GRIDHIP_EINVAL;
    if (!tc_cube_ok(B, T, F, A) || I < 1 || I > T || Nd < 1 || Nd > TC_MAX_ND || Nm < 1 || Nm > TC_MAX_NM || !tables || !vis ||
        !a1 || !a2 || !sol || !peaks || !info || !stats || rounds < 1 || rounds > GRIDHIP_TEC_MAX_ROUNDS || wj < 0 ||
        wj > TC_MAX_ND || wm < 0 || wm > TC_MAX_NM || (warm != 0 && warm != 1) ||
        !fringe_solve_args_ok(B, I, A, min_count, min_coh2, refant, niter, tol) || ((uintptr_t)vis & 15) ||
        ((uintptr_t)model_vis & 15))
        return fail(ctx, GRIDHIP_EINVAL, "tecfit: bad argument");
    const int64_t ntj0 = tc_tiles(Nd, TC_TJ), ntm0 = tc_tiles(Nm, TC_TM);
    const int64_t ntj1 = tc_tiles(2 * wj + 1, TC_TJ), ntm1 = tc_tiles(2 * wm + 1, TC_TM);
    const int64_t nt0 = ntj0 * ntm0, nt1 = ntj1 * ntm1, ntmax = nt0 > nt1 ? nt0 : nt1;
    if (!tc_cube_fits(B, T, A) || B * T > ((int64_t)1 << 31) - 1 || B * I * ntmax > 0x7fffffffLL)
        return fail(ctx, GRIDHIP_EUNSUPPORTED, "tecfit: B above 2^24, T above 2^20, A above 1024, or too many tiles");
    const size_t n = (size_t)B * T * F, tb = tc_table_bytes(F, Nd, Nm), pb = (size_t)B * I * TC_ROW * 8;
    const size_t sb = (size_t)I * A * 32, nb = (size_t)I * A * 8, ib = (size_t)B * 8;
    if (outputs_clash({{sol, sb}, {peaks, pb}, {info, nb}, {stats, 64}},
                      {{tables, tb}, {vis, n * 16}, {model_vis, n * 16}, {wt, n * 8}, {a1, ib}, {a2, ib}}))
        return fail(ctx, GRIDHIP_EINVAL, "tecfit: arrays overlap");
    GH_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    DevBuf cnt, cand, w, part, st, edges;
    GH_CHECK(cnt.alloc(ctx, sizeof(TcCount)));
    GH_CHECK(cand.alloc(ctx, (size_t)B * I * ntmax * 32));
    GH_CHECK(w.alloc(ctx, (size_t)I * B * 8));
    GH_CHECK(part.alloc(ctx, (size_t)I * 64));
    GH_CHECK(st.alloc(ctx, 128));
    GH_CHECK(edges.alloc(ctx, (size_t)I * B * 2 * sizeof(FrEdge)));
    Staged sg(ctx, dev);
    TcSearch a{};
    a.B = (int)B, a.T = (int)T, a.F = (int)F, a.A = (int)A;
    a.tables = sg.in(tables, tb);
    a.vis = reinterpret_cast<const double2 *>(sg.in(vis, n * 16));
    a.model = reinterpret_cast<const double2 *>(sg.in(model_vis, n * 16));
    a.wt = sg.in(wt, n * 8), a.a1 = sg.in(a1, ib), a.a2 = sg.in(a2, ib);
    double *dsol = sg.inout(sol, sol, sb);
    a.peaks = sg.inout(peaks, peaks, pb);
    double *dinfo = sg.inout(info, info, nb);
    stats = sg.out(stats, 64);
    a.Ib = (int)I, a.cand = cand.as<double>(), a.cnt = cnt.as<TcCount>();
    GH_CHECK(sg.status());
    FrSolve v{};
    v.B = (int)B, v.I = (int)I, v.A = (int)A, v.a1 = a.a1, v.a2 = a.a2, v.peaks = a.peaks;
    v.min_count = min_count, v.min_coh2 = min_coh2, v.refant = (int)(refant < 0 ? -1 : refant), v.niter = (int)niter, v.tol = tol;
    v.sol = dsol, v.info = dinfo, v.w = w.as<double>(), v.part = part.as<double>(), v.edges = edges.as<FrEdge>();
    double *ss = st.as<double>(), *vs = ss + 8;
    v.gate = ss;
    if (!warm) fringe_init_sol_enqueue(ctx, I * A, dsol);
    for (int64_t r = 0; r < rounds; ++r) {
        if (r == 0) {
            a.mode = 2, a.j0 = 0, a.j1 = (int)Nd, a.m0 = 0, a.m1 = (int)Nm, a.ntj = (int)ntj0, a.ntm = (int)ntm0;
            a.sol = warm ? dsol : nullptr;
        } else {
            a.mode = 1, a.wj = (int)wj, a.wm = (int)wm, a.ntj = (int)ntj1, a.ntm = (int)ntm1, a.sol = dsol;
        }
        tc_search_launch(ctx, a, I, ss);
        fringe_solve_enqueue(ctx, v, vs);
    }
    hipLaunchKernelGGL(tc_fit_stats_kernel, dim3(1), dim3(64), 0, ctx->stream, (int)T, (int)F, (int)I, (int)Nd, (int)Nm, a.tables,
                       (const double *)ss, (const double *)vs, stats);
    GH_CHECK_HIP(ctx, hipGetLastError());
    return sg.finish();
}

int tc_apply_any(gridhip_ctx *ctx, bool dev, int64_t B, int64_t T, int64_t F, int64_t A, int64_t I, const double *tables,
                 const double *sol, const int64_t *a1, const int64_t *a2, int inverse, const double *vis_in,
                 const double *wt_in, double *vis_out, double *wt_out)
{
    if (!ctx) return GRIDHIP_EINVAL;
    if (!tc_cube_ok(B, T, F, A) || I < 1 || I > T || !tables || !sol || !a1 || !a2 || !vis_in || !vis_out ||
        (inverse != 0 && inverse != 1) || ((uintptr_t)vis_in & 15) || ((uintptr_t)vis_out & 15))
        return fail(ctx, GRIDHIP_EINVAL, "apply_tec: bad argument");
    if (!tc_cube_fits(B, T, A)) return fail(ctx, GRIDHIP_EUNSUPPORTED, "apply_tec: B above 2^24, T above 2^20 or A above 1024");
    const size_t tb = dev ? (size_t)TC_HEAD * 8 : tc_host_table_bytes(tables, T, F);
    const size_t n = (size_t)B * T * F, sb = (size_t)I * A * 32, ib = (size_t)B * 8;
    if (outputs_clash({{vis_out, n * 16}, {wt_out, n * 8}},
                      {{vis_in, n * 16}, {wt_in, n * 8}, {tables, tb}, {sol, sb}, {a1, ib}, {a2, ib}}, {{0, 0}, {1, 1}}))
        return fail(ctx, GRIDHIP_EINVAL, "apply_tec: arrays overlap");
    GH_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    Staged sg(ctx, dev);
    TcApply a{};
    a.B = (int)B, a.T = (int)T, a.F = (int)F, a.A = (int)A, a.I = (int)I, a.inverse = inverse;
    a.tables = sg.in(tables, tb), a.sol = sg.in(sol, sb), a.a1 = sg.in(a1, ib), a.a2 = sg.in(a2, ib);
    // a table that does not fit leaves the outputs as they are, in the host form too: an output's block starts from the
    // output's own bytes, and is the input's block only in place
    a.vis_out = reinterpret_cast<double2 *>(sg.inout(vis_out, vis_out, n * 16));
    a.vis_in = vis_in == vis_out ? a.vis_out : reinterpret_cast<const double2 *>(sg.in(vis_in, n * 16));
    a.wt_out = sg.inout(wt_out, wt_out, n * 8);
    a.wt_in = !wt_out ? nullptr : wt_in == wt_out ? a.wt_out : sg.in(wt_in, n * 8);  // (read only for wt_out)
    GH_CHECK(sg.status());
    hipLaunchKernelGGL(tc_apply_kernel, grid_for(ctx, (int64_t)n), dim3(256), 0, ctx->stream, a);
    GH_CHECK_HIP(ctx, hipGetLastError());
    return sg.finish();
}

}  // namespace

}  // namespace gridhip

using namespace gridhip;

extern "C" {

int gridhip_tec_tables(gridhip_ctx *ctx, int64_t F, int64_t T, int64_t tint, const double *freq, double tau0, double dtau,
                       int64_t Nd, double tec0, double dtec, int64_t Nm, double *tables)
{
    return tc_tables_any(ctx, false, F, T, tint, freq, tau0, dtau, Nd, tec0, dtec, Nm, tables);
}

int gridhip_tec_tables_dev(gridhip_ctx *ctx, int64_t F, int64_t T, int64_t tint, const double *freq, double tau0, double dtau,
                           int64_t Nd, double tec0, double dtec, int64_t Nm, double *tables)
{
    return tc_tables_any(ctx, true, F, T, tint, freq, tau0, dtau, Nd, tec0, dtec, Nm, tables);
}

int gridhip_tec_search(gridhip_ctx *ctx, int64_t B, int64_t T, int64_t F, int64_t A, int64_t I, const double *tables,
                       const double *vis, const double *model_vis, const double *wt, const int64_t *a1, const int64_t *a2,
                       const double *sol, int64_t j0, int64_t j1, int64_t m0, int64_t m1, double *peaks, double *stats)
{
    return tc_search_any(ctx, false, B, T, F, A, I, tables, vis, model_vis, wt, a1, a2, sol, j0, j1, m0, m1, peaks, stats);
}

int gridhip_tec_search_dev(gridhip_ctx *ctx, int64_t B, int64_t T, int64_t F, int64_t A, int64_t I, const double *tables,
                           const double *vis, const double *model_vis, const double *wt, const int64_t *a1, const int64_t *a2,
                           const double *sol, int64_t j0, int64_t j1, int64_t m0, int64_t m1, double *peaks, double *stats)
{
    return tc_search_any(ctx, true, B, T, F, A, I, tables, vis, model_vis, wt, a1, a2, sol, j0, j1, m0, m1, peaks, stats);
}

int gridhip_tecfit(gridhip_ctx *ctx, int64_t B, int64_t T, int64_t F, int64_t A, int64_t I, int64_t Nd, int64_t Nm,
                   const double *tables, const double *vis, const double *model_vis, const double *wt, const int64_t *a1,
                   const int64_t *a2, int64_t rounds, int64_t wj, int64_t wm, double min_count, double min_coh2, int64_t refant,
                   int64_t niter, double tol, int warm, double *sol, double *peaks, double *info, double *stats)
{
    return tc_fit_any(ctx, false, B, T, F, A, I, Nd, Nm, tables, vis, model_vis, wt, a1, a2, rounds, wj, wm, min_count, min_coh2,
                      refant, niter, tol, warm, sol, peaks, info, stats);
}

int gridhip_tecfit_dev(gridhip_ctx *ctx, int64_t B, int64_t T, int64_t F, int64_t A, int64_t I, int64_t Nd, int64_t Nm,
                       const double *tables, const double *vis, const double *model_vis, const double *wt, const int64_t *a1,
                       const int64_t *a2, int64_t rounds, int64_t wj, int64_t wm, double min_count, double min_coh2,
                       int64_t refant, int64_t niter, double tol, int warm, double *sol, double *peaks, double *info,
                       double *stats)
{
    return tc_fit_any(ctx, true, B, T, F, A, I, Nd, Nm, tables, vis, model_vis, wt, a1, a2, rounds, wj, wm, min_count, min_coh2,
                      refant, niter, tol, warm, sol, peaks, info, stats);
}

int gridhip_apply_tec(gridhip_ctx *ctx, int64_t B, int64_t T, int64_t F, int64_t A, int64_t I, const double *tables,
                      const double *sol, const int64_t *a1, const int64_t *a2, int inverse, const double *vis_in,
                      const double *wt_in, double *vis_out, double *wt_out)
{
    return tc_apply_any(ctx, false, B, T, F, A, I, tables, sol, a1, a2, inverse, vis_in, wt_in, vis_out, wt_out);
}

int gridhip_apply_tec_dev(gridhip_ctx *ctx, int64_t B, int64_t T, int64_t F, int64_t A, int64_t I, const double *tables,
                          const double *sol, const int64_t *a1, const int64_t *a2, int inverse, const double *vis_in,
                          const double *wt_in, double *vis_out, double *wt_out)
{
    return tc_apply_any(ctx, true, B, T, F, A, I, tables, sol, a1, a2, inverse, vis_in, wt_in, vis_out, wt_out);
}

int gridhip_tec_tile(int64_t *out)
{
    if (!out) return GRIDHIP_EINVAL;
    out[0] = TC_TJ, out[1] = TC_TM, out[2] = TC_KC;
    return GRIDHIP_OK;
}

}  // extern "C"
