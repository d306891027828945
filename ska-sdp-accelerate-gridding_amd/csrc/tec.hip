// Dispersive delay (TEC) calibration (include/gridhip.h, "dispersive delay (TEC) calibration"): a search per baseline and
// solution interval over a grid of delays and orthogonalised TEC cells, the antenna fit of fringe_solve.hip, and the apply
// step.
//
//     gridhip_tec_tables   tc_head_kernel (one work-group: the checks, s, the head), tc_fill_kernel (one thread per entry)
//     gridhip_tec_search   dl_zero_kernel, tc_search_kernel, tc_refine_kernel, dl_search_stats_kernel<TcSearch>
//     gridhip_tecfit       dl_fit_any<TcMod>: [the solve's init]; per round the four above and the two of the solve;
//                          dl_fit_stats_kernel<TcMod>
//     gridhip_apply_tec    dl_apply_kernel<TcMod> (one thread per sample)
// The dl_ names are delay_common.h's, which fringe.hip uses alike: the rounded arithmetic, the counters, the sample before
// its derotation, the reduction to a candidate, the ends of the refinement, the apply step, the host rules and the fit
// driver.  This file owns the table, the window, the derotation and the two large kernels, and TcMod, which tells the
// shared templates about them.
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
#include "delay_common.h"

#pragma clang fp contract(off)

namespace gridhip {

namespace {

constexpr int TC_THREADS = 256;
constexpr int TC_RJ = 2;                                  // delays of a lane
constexpr int TC_TJ = TC_THREADS * TC_RJ;                 // delays of a work-group
constexpr int TC_TM = 8;                                  // TEC cells of a work-group
constexpr int TC_KC = 4;                                  // channels of a staged chunk of a full tile
constexpr int TC_ES = TC_KC * TC_TJ;                      // the Ef entries staged at a time
constexpr int TC_KMAX = TC_ES / 64;                       // channels of a staged chunk of the narrowest tile
constexpr int TC_HEAD = DL_HEAD, TC_ROW = DL_ROW;
constexpr int TC_MAX_F = GRIDHIP_TEC_MAX_CHANNELS, TC_MAX_ND = GRIDHIP_TEC_MAX_DELAYS, TC_MAX_NM = GRIDHIP_TEC_MAX_CELLS;

struct TcHead {
    bool ok;
    int F, T, tint, I, Nd, Nm;
    double tau0, dtau, tec0, dtec;
    const double2 *Ef, *Em;
    const double *af, *cf;
};

// the head of a table, and whether it fits a cube of T time steps and F channels
__device__ __forceinline__ TcHead tc_head(const double *tb, int T, int F)
{
    TcHead h;
    h.ok = tb[0] == 1.0 && tb[1] == (double)F && tb[2] == (double)T && T >= 1 && dl_int_in(tb[3], 1, T) &&
           dl_int_in(tb[5], 1, TC_MAX_ND) && dl_int_in(tb[6], 1, TC_MAX_NM) && F >= 1 && F <= TC_MAX_F;
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

// z_f = -(kappa (1 / nu_f - 1 / nu0)), every operation rounded
__device__ __forceinline__ double tc_z(double nu, double nu0) { return -(GRIDHIP_TEC_KAPPA * (1.0 / nu - 1.0 / nu0)); }

__global__ void __launch_bounds__(256)
    tc_head_kernel(int F, int T, int tint, int Nd, int Nm, const double *__restrict__ freq, double tau0, double dtau,
                   double tec0, double dtec, double *__restrict__ tables)
{
    if (blockIdx.x != 0) return;
    int bad = 0;  // the one work-group shares the scan of freq
    for (int i = threadIdx.x; i < F; i += blockDim.x) bad |= !(dl_finite(freq[i]) && freq[i] > 0.0);
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
    const bool ok = !bad && dl_finite(tau0) && dl_finite(dtau) && dl_finite(tec0) && dl_finite(dtec) && dtau > 0.0 &&
                    dtec > 0.0 && dl_finite(nu0) && dl_finite(s);
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
                e = dl_phasor(tau0 + (double)j * dtau, freq[f] - nu0);
            }
            Ef[2 * i] = e.x, Ef[2 * i + 1] = -e.y;
        } else if (i < nF + nM) {
            const int64_t k = i - nF;
            double2 e = make_double2(0.0, 0.0);
            if (valid) {
                const int f = (int)(k / Nm), m = (int)(k % Nm);
                const double a = freq[f] - nu0;
                e = dl_phasor(tec0 + (double)m * dtec, tc_z(freq[f], nu0) - s * a);
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

struct TcSearch : DlSearch {
    // mode 0: the cells [j0, j1) x [m0, m1); 1: those within (wj, wm) of the grid's zero; 2: the whole grid, j1 = Nd, m1 = Nm
    int j0, j1, m0, m1, wj, wm;
    int ntj, ntm;  // the tiles launched along either axis: cand is [B][Ib][ntj * ntm][4]
    __device__ bool fits() const;
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

__device__ __forceinline__ bool TcSearch::fits() const
{
    int j0, j1, m0, m1;
    return tc_window(tc_head(tables, T, F), *this, &j0, &j1, &m0, &m1);
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
        r.d = dl_mulc(make_double2(sp[2], sp[3]), make_double2(sq[2], sq[3]));
    }
    return r;
}

// Dfm[f] = ph(tau_p - tau_q, a_f) ph(tec_p - tec_q, c_f)
__device__ __forceinline__ double2 tc_dfm(const TcHead &h, const TcDerot &r, int f)
{
    return dl_mul(dl_phasor(r.dtau, h.af[f]), dl_phasor(r.dtec, h.cf[f]));
}

// X' of the sample at `at`: dl_sample's, derotated as (x conj(d)) conj(Df Dm)
__device__ __forceinline__ double2 tc_sample(const TcSearch &a, int64_t at, const TcDerot &r, double2 dfm, bool *flagged)
{
    return dl_sample(a, at, flagged, [&](double2 x) { return r.on ? dl_mulc(dl_mulc(x, r.d), dfm) : x; });
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
                for (int mm = 0; mm < RM; ++mm) pr[mm] = dl_mul(Ms[kc * TC_TM + mm], x);
#pragma unroll
                for (int r = 0; r < TC_RJ; ++r) {
                    if (!on[r]) continue;
                    const double2 e = Es[kc * stride + jl + r * 64];
#pragma unroll
                    for (int mm = 0; mm < RM; ++mm) dl_mac(acc[r][mm], e, pr[mm]);
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
            if (j < j1 && m < m1 && dl_ahead(P, j, m, *bp, *bj, *bm)) *bp = P, *bj = j, *bm = m;
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
        if (tid == 0) dl_put_cand(c, -1.0, -1, -1);
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
    dl_group_best<TC_THREADS / 64>(tid, bp, bj, bm, rp, rj, rm);
    if (tid == 0) dl_put_cand(c, bp, bj, bm);
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
    double out[TC_ROW] = {};
    dl_row_none(out);
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
                        bad = bad || !(dl_finite(x.x) && dl_finite(x.y));
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
        double bp;
        int bj, bm;
        dl_best_tile(a.cand + ((int64_t)b * a.Ib + i) * ((int64_t)a.ntj * a.ntm) * 4, (j1 - j0 + TC_TJ - 1) / TC_TJ,
                     (m1 - m0 + TC_TM - 1) / TC_TM, a.ntm, &bp, &bj, &bm);
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
                    dl_mac(S, h.Ef[(int64_t)f * h.Nd + j], dl_mul(h.Em[(int64_t)f * h.Nm + m], Xs[f]));
            }
            // (the recomputed power of a selected cell is the candidate's: never a NaN)
            if (!dl_peak_row(out, bj, bm, inj, inm, S, N, nu, h.tau0, h.dtau, h.tec0, h.dtec)) code = 2;
        }
    }
    if (lane == 0) dl_put_row(a.cnt, row, out, code, nflag);
}

size_t tc_table_bytes(int64_t F, int64_t Nd, int64_t Nm) { return (size_t)GRIDHIP_TEC_TABLE_DOUBLES(F, Nd, Nm) * 8; }

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

int64_t tc_tiles(int64_t n, int64_t tile) { return (n + tile - 1) / tile; }

struct TcMod {  // this module as delay_common.h's templates see it
    typedef TcSearch Search;
    typedef TcHead Head;
    static constexpr const char *fit_name = "tecfit", *apply_name = "apply_tec";
    static constexpr int MAX_F = TC_MAX_F, MAX_N1 = TC_MAX_ND, MAX_N2 = TC_MAX_NM, MAX_ROUNDS = GRIDHIP_TEC_MAX_ROUNDS;

    static __device__ __forceinline__ TcHead head(const double *tb, int T, int F) { return tc_head(tb, T, F); }

    // v (d (Df Dm)) of the solutions sp and sq, or v conj(..): Df Dm is one factor, as in tc_dfm
    static __device__ __forceinline__ double2 rotate(const TcHead &h, int f, int, const double *sp, const double *sq, int inverse,
                                                     double2 v)
    {
        const double2 d = dl_mulc(make_double2(sp[2], sp[3]), make_double2(sq[2], sq[3]));
        const double2 dfm = dl_mul(dl_phasor(sp[0] - sq[0], h.af[f]), dl_phasor(sp[1] - sq[1], h.cf[f]));
        return inverse ? dl_mulc(dl_mulc(v, d), dfm) : dl_mul(dl_mul(v, d), dfm);
    }

    static __device__ __forceinline__ bool fit_steps(const double *tables, int T, int F, int I, int Nd, int Nm, double *d1, double *d2)
    {
        const TcHead h = tc_head(tables, T, F);
        *d1 = h.dtau, *d2 = h.dtec;
        return h.ok && h.I == I && h.Nd == Nd && h.Nm == Nm;
    }

    static size_t table_bytes(int64_t F, int64_t, int64_t Nd, int64_t Nm) { return tc_table_bytes(F, Nd, Nm); }

    static size_t host_table_bytes(const double *tables, int64_t T, int64_t F)
    {
        return dl_host_head_fits(tables, T, F, T, TC_MAX_ND, TC_MAX_NM) ? tc_table_bytes(F, (int64_t)tables[5], (int64_t)tables[6])
                                                                        : (size_t)TC_HEAD * 8;
    }

    // (every field is set in every round: tc_window reads the half-widths in mode 1 alone and the cells in the other modes)
    static void round(TcSearch &a, bool whole, int64_t Nd, int64_t Nm, int64_t wj, int64_t wm)
    {
        a.mode = whole ? 2 : 1, a.j0 = 0, a.j1 = (int)Nd, a.m0 = 0, a.m1 = (int)Nm, a.wj = (int)wj, a.wm = (int)wm;
        a.ntj = (int)tc_tiles(whole ? Nd : 2 * wj + 1, TC_TJ), a.ntm = (int)tc_tiles(whole ? Nm : 2 * wm + 1, TC_TM);
    }
    static int64_t tiles(const TcSearch &a) { return (int64_t)a.ntj * a.ntm; }
    static int64_t groups(const TcSearch &a, int64_t B, int64_t I) { return B * I * tiles(a); }
    static void search_launch(gridhip_ctx *ctx, const TcSearch &a, int64_t nI, double *stats)
    {
        hipLaunchKernelGGL(dl_zero_kernel, dim3(1), dim3(64), 0, ctx->stream, a.cnt);
        hipLaunchKernelGGL(tc_search_kernel, dim3((unsigned)groups(a, a.B, nI)), dim3(TC_THREADS), 0, ctx->stream, a);
        hipLaunchKernelGGL(tc_refine_kernel, dim3((unsigned)((int64_t)a.B * nI)), dim3(64), 0, ctx->stream, a);
        hipLaunchKernelGGL(dl_search_stats_kernel<TcSearch>, dim3(1), dim3(64), 0, ctx->stream, a, stats);
    }
};

int tc_search_any(gridhip_ctx *ctx, bool dev, int64_t B, int64_t T, int64_t F, int64_t A, int64_t I, const double *tables,
                  const double *vis, const double *model_vis, const double *wt, const int64_t *a1, const int64_t *a2,
                  const double *sol, int64_t j0, int64_t j1, int64_t m0, int64_t m1, double *peaks, double *stats)
{
    if (!ctx) return GRIDHIP_EINVAL;
    if (!dl_cube_ok(B, T, F, A, TC_MAX_F) || I < 1 || I > T || !tables || !vis || !a1 || !a2 || !peaks || !stats || j0 < 0 ||
        j0 >= j1 || j1 > TC_MAX_ND || m0 < 0 || m0 >= m1 || m1 > TC_MAX_NM || ((uintptr_t)vis & 15) || ((uintptr_t)model_vis & 15))
        return fail(ctx, GRIDHIP_EINVAL, "tec_search: bad argument");
    if (!dl_cube_fits(B, T, A) || B * T > ((int64_t)1 << 31) - 1)
        return fail(ctx, GRIDHIP_EUNSUPPORTED, "tec_search: B above 2^24, T above 2^20, A above 1024 or B T above 2^31 - 1");
    const size_t tb = dev ? (size_t)TC_HEAD * 8 : TcMod::host_table_bytes(tables, T, F);
    const int64_t ntj = tc_tiles(j1 - j0, TC_TJ), ntm = tc_tiles(m1 - m0, TC_TM);
    if (B * I * ntj * ntm > 0x7fffffffLL) return fail(ctx, GRIDHIP_EUNSUPPORTED, "tec_search: more than 2^31 - 1 tiles");
    const size_t n = (size_t)B * T * F, pb = (size_t)B * I * TC_ROW * 8, sb = (size_t)I * A * 32, ib = (size_t)B * 8;
    if (outputs_clash({{peaks, pb}, {stats, 64}},
                      {{tables, tb}, {vis, n * 16}, {model_vis, n * 16}, {wt, n * 8}, {a1, ib}, {a2, ib}, {sol, sb}}))
        return fail(ctx, GRIDHIP_EINVAL, "tec_search: arrays overlap");
    GH_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    DevBuf cnt, cand;
    GH_CHECK(cnt.alloc(ctx, sizeof(DlCount)));
    GH_CHECK(cand.alloc(ctx, (size_t)B * I * ntj * ntm * 32));
    Staged sg(ctx, dev);
    TcSearch a{};
    dl_stage_search(sg, a, B, T, F, A, I, tables, tb, vis, model_vis, wt, a1, a2, peaks, cand, cnt);
    a.sol = sg.in(sol, sb);
    stats = sg.out(stats, 64);
    a.mode = 0, a.j0 = (int)j0, a.j1 = (int)j1, a.m0 = (int)m0, a.m1 = (int)m1, a.ntj = (int)ntj, a.ntm = (int)ntm;
    GH_CHECK(sg.status());
    TcMod::search_launch(ctx, a, I, stats);
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
    return dl_fit_any<TcMod>(ctx, false, B, T, F, A, I, Nd, Nm, tables, vis, model_vis, wt, a1, a2, rounds, wj, wm, min_count,
                             min_coh2, refant, niter, tol, warm, sol, peaks, info, stats);
}

int gridhip_tecfit_dev(gridhip_ctx *ctx, int64_t B, int64_t T, int64_t F, int64_t A, int64_t I, int64_t Nd, int64_t Nm,
                       const double *tables, const double *vis, const double *model_vis, const double *wt, const int64_t *a1,
                       const int64_t *a2, int64_t rounds, int64_t wj, int64_t wm, double min_count, double min_coh2,
                       int64_t refant, int64_t niter, double tol, int warm, double *sol, double *peaks, double *info,
                       double *stats)
{
    return dl_fit_any<TcMod>(ctx, true, B, T, F, A, I, Nd, Nm, tables, vis, model_vis, wt, a1, a2, rounds, wj, wm, min_count,
                             min_coh2, refant, niter, tol, warm, sol, peaks, info, stats);
}

int gridhip_apply_tec(gridhip_ctx *ctx, int64_t B, int64_t T, int64_t F, int64_t A, int64_t I, const double *tables,
                      const double *sol, const int64_t *a1, const int64_t *a2, int inverse, const double *vis_in,
                      const double *wt_in, double *vis_out, double *wt_out)
{
    return dl_apply_any<TcMod>(ctx, false, B, T, F, A, I, tables, sol, a1, a2, inverse, vis_in, wt_in, vis_out, wt_out);
}

int gridhip_apply_tec_dev(gridhip_ctx *ctx, int64_t B, int64_t T, int64_t F, int64_t A, int64_t I, const double *tables,
                          const double *sol, const int64_t *a1, const int64_t *a2, int inverse, const double *vis_in,
                          const double *wt_in, double *vis_out, double *wt_out)
{
    return dl_apply_any<TcMod>(ctx, true, B, T, F, A, I, tables, sol, a1, a2, inverse, vis_in, wt_in, vis_out, wt_out);
}

int gridhip_tec_tile(int64_t *out)
{
    if (!out) return GRIDHIP_EINVAL;
    out[0] = TC_TJ, out[1] = TC_TM, out[2] = TC_KC;
    return GRIDHIP_OK;
}

}  // extern "C"
