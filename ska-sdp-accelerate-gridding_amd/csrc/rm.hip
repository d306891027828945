// Rotation-measure synthesis and RM-CLEAN (include/gridhip.h, "rotation-measure synthesis"): per line of sight (LOS) the
// complex polarisation P(lambda^2) = Q + iU of C channels becomes the Faraday dispersion function F(phi) at J depths, and
// a Hogbom loop along phi with the RM spread function deconvolves every LOS on its own.
//
//     gridhip_rm_tables    rm_head_kernel (one thread: the checks of lam2 and the weights, the two sums, lam0^2, K)
//                          rm_fill_kernel (one thread per entry of E, R and G; the only sum is R's, over C channels)
//     gridhip_rmsynth      rm_zero_kernel, rm_synth_kernel, rm_synth_stats_kernel
//     gridhip_rmclean      rm_zero_kernel, rm_clean_kernel<NR, STAGE>, rm_clean_stats_kernel
// Every kernel that reads a table judges its head itself (valid, C, J) and leaves at once when it does not fit; the last
// kernel of a call writes the 8 stats.  Nothing is read back, nothing depends on the data but the length of a wave's loop.
//
// THE SYNTHESIS KERNEL.  cube[j][m] = sum_c E[c][j] (Q[c][m] + i U[c][m]) is a [J x C] . [C x M] complex product in plain
// fp64 VALU.  A work-group of 256 threads owns RM_TJ = 64 depths x RM_TM = 64 LOS; lane (ty, tx) = (tid / 16, tid % 16)
// keeps the 4 x 4 complex accumulators of the depths 4 ty .. 4 ty + 3 and the LOS 4 tx .. 4 tx + 3: 64 VGPRs, with the
// operands about 110, four waves per SIMD.  A chunk of RM_KC = 16 channels of E (64 depths, 16 KB) and of Q and U (64 LOS,
// 8 KB each) is staged in LDS, 32 KB per work-group; Q and U are read as the two real cubes they are, 512 B of a row at a
// time.  A k-step reads 128 B of LDS per lane (E broadcast over the 16 lanes of a ty) for 128 fp64 instructions: the
// vector pipe binds, not the LDS.  Every output element belongs to one lane, which adds its channels in ascending order,
// unfused (8 instructions per complex multiply-add where a fused one takes 4): the determinism argument.  The depth tile
// is the fast index of the grid, so the J / 64 work-groups that read the same rows of Q and U run together.
//
// THE CLEAN KERNEL.  One wave per LOS, a work-group of four waves owns four consecutive LOS (work-groups stride over the
// groups).  Depth j lives in register j / 64 of lane j % 64: NR = 1, 2, 4 or 8 complex residuals and as many model values
// per lane, all in registers.  R and G lie in LDS (24 KB), staged once per work-group.  The arg-max is a butterfly over
// (p, j) pairs; in the subtraction consecutive lanes read consecutive entries of R; the restore walks the set bits of a
// ballot of the non-zero model values and broadcasts each from its lane.  The loop's length differs between waves and
// never within one.  Reading cube[j][m] is a strided read per lane; STAGE = false lets the four waves of a group read
// their 16-byte pieces of the same 64 bytes directly, STAGE = true has the group read 64 depths x 4 LOS with consecutive
// threads along m and hands the columns over through LDS (option "rm_stage").  Measured at 1024^2 LOS, J = 256, 100
// components: equal within the spread when every loop has the same length, and the direct read 2.5 to
// 4 % faster when the lengths differ - staged, the four waves of a group wait for each other at every LOS.  Direct is
// the default.
// Counts go to a small block by one integer atomic per wave and counter, at the end of the kernel.
#include "common.h"
#include "imaging.h"

#pragma clang fp contract(off)

namespace gridhip {

namespace {

typedef unsigned long long u64;

constexpr int RM_THREADS = 256;
constexpr int RM_TM = 64, RM_TJ = 64, RM_KC = 16;  // the synthesis tile: LOS, depths, channels of a chunk
constexpr int RM_GROUP = RM_THREADS / 64;          // LOS of a work-group of the clean
constexpr int RM_MAX_C = GRIDHIP_RM_MAX_CHANNELS, RM_MAX_J = GRIDHIP_RM_MAX_DEPTHS, RM_HEAD = GRIDHIP_RM_HEAD;
constexpr double RM_INV_PI = 0.3183098861837907;
constexpr double RM_FOUR_LN2 = 2.772588722239781;  // 4 ln 2
static_assert(RM_TM * RM_KC == 4 * RM_THREADS && RM_TJ == RM_TM, "the synthesis kernel's staging");

struct RmCount {  // the counters of one call
    u64 bad, iters, by_niter, by_level;
    u64 pad[4];
};

__device__ __forceinline__ bool rm_finite(double x) { return __builtin_isfinite(x); }

// kw exp(-2 i x a): t = (x a) / pi reduced to r = t - rint(t) (exact), then sincospi(2 r)
__device__ __forceinline__ void rm_phasor(double x, double a, double kw, double *re, double *im)
{
    const double t = (x * a) * RM_INV_PI;
    const double r = t - rint(t);
    double sn, cs;
    sincospi(2.0 * r, &sn, &cs);
    *re = kw * cs;
    *im = -(kw * sn);
}

// does the table's head fit a call with these C and J?  (C < 0: any C in range; *c_out gets the head's)
__device__ __forceinline__ bool rm_head_ok(const double *head, int C, int J, int *c_out)
{
    const double hc = head[1];
    const bool ok = head[0] == 1.0 && hc >= 1.0 && hc <= (double)RM_MAX_C && hc == (double)(int)hc && head[2] == (double)J &&
                    (C < 0 || hc == (double)C);
    *c_out = ok ? (int)hc : 1;
    return ok;
}

__global__ void rm_head_kernel(int C, int J, const double *__restrict__ lam2, const double *__restrict__ w, double phi0,
                               double dphi, double fwhm, double *__restrict__ tables)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    bool ok = true;
    double sw = 0.0, swl = 0.0;
    for (int c = 0; c < C; ++c) {
        const double wc = w ? w[c] : 1.0, l = lam2[c];
        ok = ok && rm_finite(l) && rm_finite(wc) && wc >= 0.0;
        sw = sw + wc;
        swl = swl + wc * l;
    }
    ok = ok && rm_finite(sw) && sw > 0.0 && rm_finite(swl);
    for (int i = 0; i < RM_HEAD; ++i) tables[i] = 0.0;
    tables[0] = ok ? 1.0 : 0.0;
    tables[1] = (double)C, tables[2] = (double)J, tables[3] = phi0, tables[4] = dphi, tables[8] = fwhm;
    if (ok) tables[5] = swl / sw, tables[6] = 1.0 / sw, tables[7] = sw;
}

__global__ void __launch_bounds__(256)
    rm_fill_kernel(int C, int J, const double *__restrict__ lam2, const double *__restrict__ w, double *tables)
{
    const bool valid = tables[0] == 1.0;
    const double phi0 = tables[3], dphi = tables[4], lam0 = tables[5], K = tables[6], fwhm = tables[8];
    const int64_t nE = (int64_t)C * J, nL = 2 * (int64_t)J - 1, total = nE + 2 * nL;
    double *E = tables + RM_HEAD, *R = E + 2 * nE, *G = R + 2 * nL;
    const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, step = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = i0; i < total; i += step) {
        if (i < nE) {
            double re = 0.0, im = 0.0;
            if (valid) {
                const int c = (int)(i / J), j = (int)(i % J);
                const double phi = phi0 + (double)j * dphi;
                rm_phasor(phi, lam2[c] - lam0, K * (w ? w[c] : 1.0), &re, &im);
            }
            E[2 * i] = re, E[2 * i + 1] = im;
        } else if (i < nE + nL) {
            const int64_t k = i - nE;
            double sre = 0.0, sim = 0.0;
            if (valid) {
                const double lag = (double)(k - (J - 1)) * dphi;
                for (int c = 0; c < C; ++c) {
                    double re, im;
                    rm_phasor(lag, lam2[c] - lam0, K * (w ? w[c] : 1.0), &re, &im);
                    sre = sre + re;
                    sim = sim + im;
                }
            }
            R[2 * k] = sre, R[2 * k + 1] = sim;
        } else {
            const int64_t k = i - nE - nL;
            double g = 0.0;
            if (valid) {
                const double x = ((double)(k - (J - 1)) * dphi) / fwhm;
                g = exp(-(RM_FOUR_LN2 * (x * x)));
            }
            G[k] = g;
        }
    }
}

__global__ void rm_zero_kernel(RmCount *cnt)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) *cnt = RmCount{};
}

__global__ void __launch_bounds__(RM_THREADS)
    rm_synth_kernel(int64_t M, int C, int J, int ndt, const double *__restrict__ tables, const double *__restrict__ Q,
                    const double *__restrict__ U, double2 *__restrict__ cube, RmCount *cnt)
{
    __shared__ double2 Es[RM_KC * RM_TJ];
    __shared__ double Qs[RM_KC * RM_TM], Us[RM_KC * RM_TM];
    __shared__ int bad_s[RM_TM];
    int c_head;
    if (!rm_head_ok(tables, C, J, &c_head)) return;
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int64_t lt = (int64_t)blockIdx.x / ndt;
    const int dt = (int)((int64_t)blockIdx.x - lt * ndt);
    const int64_t m0 = lt * RM_TM;
    const int j0 = dt * RM_TJ;
    const double *E = tables + RM_HEAD;
    double are[4][4], aim[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int l = 0; l < 4; ++l) are[i][l] = 0.0, aim[i][l] = 0.0;
    if (tid < RM_TM) bad_s[tid] = 0;
    for (int c0 = 0; c0 < C; c0 += RM_KC) {
        const int nk = C - c0 < RM_KC ? C - c0 : RM_KC;
        __syncthreads();  // (bad_s zeroed; the chunk before has been read)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int idx = tid + r * RM_THREADS, kc = idx >> 6, x = idx & 63;
            double q = 0.0, u = 0.0, ere = 0.0, eim = 0.0;
            if (kc < nk) {
                if (m0 + x < M) {
                    const int64_t at = (int64_t)(c0 + kc) * M + m0 + x;
                    q = Q[at], u = U[at];
                    if (!(rm_finite(q) && rm_finite(u))) bad_s[x] = 1;  // (every writer writes 1)
                }
                if (j0 + x < J) {
                    const double *e = E + 2 * ((int64_t)(c0 + kc) * J + j0 + x);
                    ere = e[0], eim = e[1];
                }
            }
            Qs[idx] = q, Us[idx] = u, Es[idx] = make_double2(ere, eim);
        }
        __syncthreads();
        for (int kc = 0; kc < nk; ++kc) {
            double q[4], u[4];
            double2 e[4];
#pragma unroll
            for (int l = 0; l < 4; ++l) q[l] = Qs[kc * RM_TM + tx * 4 + l], u[l] = Us[kc * RM_TM + tx * 4 + l];
#pragma unroll
            for (int i = 0; i < 4; ++i) e[i] = Es[kc * RM_TJ + ty * 4 + i];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int l = 0; l < 4; ++l) {
                    are[i][l] = are[i][l] + (e[i].x * q[l] - e[i].y * u[l]);
                    aim[i][l] = aim[i][l] + (e[i].x * u[l] + e[i].y * q[l]);
                }
        }
    }
    __syncthreads();  // (bad_s is final)
    const double nan = __builtin_nan("");
    unsigned int nbad = 0u;
#pragma unroll
    for (int l = 0; l < 4; ++l) {
        const int64_t m = m0 + tx * 4 + l;
        if (m >= M) continue;
        const bool bad = bad_s[tx * 4 + l] != 0;
        if (bad && ty == 0 && dt == 0) nbad += 1u;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int j = j0 + ty * 4 + i;
            if (j < J) cube[(int64_t)j * M + m] = bad ? make_double2(nan, nan) : make_double2(are[i][l], aim[i][l]);
        }
    }
    if (dt == 0) {  // (the same for every thread)
        for (int o = 32; o > 0; o >>= 1) nbad += __shfl_down(nbad, o);
        if ((tid & 63) == 0 && nbad) atomicAdd(&cnt->bad, (u64)nbad);
    }
}

__global__ void rm_synth_stats_kernel(int C, int J, const double *__restrict__ tables, const RmCount *cnt,
                                      double *__restrict__ stats)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    int c_head;
    const bool ok = rm_head_ok(tables, C, J, &c_head);
    for (int i = 0; i < GRIDHIP_RM_STATS; ++i) stats[i] = 0.0;
    if (ok)
        stats[0] = (double)cnt->bad;
    else
        stats[7] = 1.0;
}

struct RmClean {
    int64_t M;
    int J;
    const double *tables;
    double2 *cube, *model;
    double gain, threshold, nsigma;
    const double *noise;
    int64_t niter;
    int restore;
    double *maps;
    RmCount *cnt;
};

// L = max(threshold, nsigma * sigma) as gridhip_clean_auto takes it; *bad: nsigma > 0 and sigma is NaN
__device__ __forceinline__ double rm_level(double threshold, double nsigma, const double *noise, bool *bad)
{
    double L = threshold;
    *bad = false;
    if (nsigma > 0.0) {
        const double sigma = *noise;
        if (sigma != sigma) {
            *bad = true;
            return sigma;
        }
        const double a = nsigma * sigma;
        L = a > L ? a : L;
    }
    return L;
}

// the value of depth j (the same in every lane, 0 <= j) out of the registers it is spread over
template <int NR>
__device__ __forceinline__ double rm_pick(const double (&v)[NR], int j)
{
    const int r = j >> 6;
    double x = 0.0;
#pragma unroll
    for (int i = 0; i < NR; ++i)
        if (i == r) x = v[i];
    return __shfl(x, j & 63);
}

// the depth of the largest p = re^2 + im^2, ties to the lowest depth, a NaN never; (-1, -1) when every p is NaN
template <int NR>
__device__ __forceinline__ void rm_argmax(const double (&re)[NR], const double (&im)[NR], int J, int lane, double *p_out,
                                          int *j_out)
{
    double bp = -1.0;
    int bj = -1;
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        const int j = r * 64 + lane;
        const double p = re[r] * re[r] + im[r] * im[r];
        if (j < J && p > bp) bp = p, bj = j;
    }
    for (int o = 32; o > 0; o >>= 1) {
        const double q = __shfl_xor(bp, o);
        const int k = __shfl_xor(bj, o);
        if (q > bp || (q == bp && k < bj)) bp = q, bj = k;
    }
    *p_out = bp, *j_out = bj;
}

// column m = base + wave of src[J][M] into the registers of the wave (0 beyond J and M)
template <int NR, bool STAGE>
__device__ __forceinline__ void rm_load(const double2 *src, int64_t M, int J, int64_t base, double2 *Ts, double (&re)[NR],
                                        double (&im)[NR])
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        double2 v = make_double2(0.0, 0.0);
        if (r * 64 < J) {  // (the same for every thread)
            if (STAGE) {
                const int d = tid >> 2, l = tid & 3, j = r * 64 + d;
                double2 t = make_double2(0.0, 0.0);
                if (j < J && base + l < M) t = src[(int64_t)j * M + base + l];
                __syncthreads();  // (the pass before has been read)
                Ts[l * 64 + d] = t;
                __syncthreads();
                v = Ts[wave * 64 + lane];
            } else {
                const int j = r * 64 + lane;
                if (j < J && base + wave < M) v = src[(int64_t)j * M + base + wave];
            }
        }
        re[r] = v.x, im[r] = v.y;
    }
}

// the reverse; mine: whether this wave's LOS is written; STAGE: wr[l] holds that for LOS base + l (LDS, set by its wave
// before the call, behind a barrier)
template <int NR, bool STAGE>
__device__ __forceinline__ void rm_store(double2 *dst, int64_t M, int J, int64_t base, double2 *Ts, const int *wr, bool mine,
                                         const double (&re)[NR], const double (&im)[NR])
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        if (r * 64 >= J) continue;  // (the same for every thread)
        if (STAGE) {
            const int d = tid >> 2, l = tid & 3, j = r * 64 + d;
            __syncthreads();  // (the pass before has been read)
            Ts[wave * 64 + lane] = make_double2(re[r], im[r]);
            __syncthreads();
            if (j < J && base + l < M && wr[l]) dst[(int64_t)j * M + base + l] = Ts[l * 64 + d];
        } else {
            const int j = r * 64 + lane;
            if (j < J && mine) dst[(int64_t)j * M + base + wave] = make_double2(re[r], im[r]);
        }
    }
}

template <int NR, bool STAGE>
__global__ void __launch_bounds__(RM_THREADS) rm_clean_kernel(RmClean a)
{
    __shared__ double2 Rs[2 * RM_MAX_J - 1];
    __shared__ double Gs[2 * RM_MAX_J - 1];
    __shared__ double2 Ts[STAGE ? RM_THREADS : 1];  // (the hand-over tile and the write flags of the staged variant)
    __shared__ int wr[RM_GROUP];
    const int J = a.J, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int C;
    if (!rm_head_ok(a.tables, -1, J, &C)) return;
    bool nan_sigma;
    const double L = rm_level(a.threshold, a.nsigma, a.noise, &nan_sigma);
    if (nan_sigma) return;
    const double L2 = L * L;
    const double phi0 = a.tables[3], dphi = a.tables[4];
    {
        const double *R = a.tables + RM_HEAD + 2 * (int64_t)C * J, *G = R + 2 * (2 * J - 1);
        for (int k = tid; k < 2 * J - 1; k += RM_THREADS) Rs[k] = make_double2(R[2 * k], R[2 * k + 1]), Gs[k] = G[k];
    }
    __syncthreads();
    const double nan = __builtin_nan("");
    u64 n_bad = 0, n_it = 0, n_niter = 0, n_level = 0;
    for (int64_t base = (int64_t)blockIdx.x * RM_GROUP; base < a.M; base += (int64_t)gridDim.x * RM_GROUP) {
        const int64_t m = base + wave;
        const bool live = m < a.M;
        double re[NR], im[NR], mre[NR], mim[NR];
        rm_load<NR, STAGE>(a.cube, a.M, J, base, Ts, re, im);
        if (a.model) {
            rm_load<NR, STAGE>(a.model, a.M, J, base, Ts, mre, mim);
        } else {
#pragma unroll
            for (int r = 0; r < NR; ++r) mre[r] = 0.0, mim[r] = 0.0;
        }
        bool fin = true;
#pragma unroll
        for (int r = 0; r < NR; ++r) fin = fin && rm_finite(re[r]) && rm_finite(im[r]);  // (0 beyond J)
        const bool good = live && __all(fin);
        if (good) {
            int64_t it = 0;
            int reason;
            for (;;) {
                double pk;
                int k;
                rm_argmax<NR>(re, im, J, lane, &pk, &k);
                if (pk <= L2) {
                    reason = 1;
                    break;
                }
                if (it >= a.niter) {
                    reason = 0;
                    break;
                }
                const double fr = a.gain * rm_pick<NR>(re, k), fi = a.gain * rm_pick<NR>(im, k);
                const int kr = k >> 6;
#pragma unroll
                for (int r = 0; r < NR; ++r) {
                    if (r == kr && lane == (k & 63)) mre[r] = mre[r] + fr, mim[r] = mim[r] + fi;
                    const int j = r * 64 + lane;
                    if (j < J) {
                        const double2 q = Rs[j - k + J - 1];
                        re[r] = re[r] - (fr * q.x - fi * q.y);
                        im[r] = im[r] - (fr * q.y + fi * q.x);
                    }
                }
                ++it;
            }
            if (a.restore) {
#pragma unroll
                for (int r = 0; r < NR; ++r) {
                    u64 mask = __ballot(mre[r] != 0.0 || mim[r] != 0.0);  // (0 beyond J)
                    while (mask) {
                        const int l = __builtin_ctzll(mask);
                        mask &= mask - 1;
                        const int k = r * 64 + l;
                        const double mr = __shfl(mre[r], l), mi = __shfl(mim[r], l);
#pragma unroll
                        for (int s = 0; s < NR; ++s) {
                            const int j = s * 64 + lane;
                            if (j < J) {
                                const double g = Gs[j - k + J - 1];
                                re[s] = re[s] + mr * g;
                                im[s] = im[s] + mi * g;
                            }
                        }
                    }
                }
            }
            double ps;
            int js;
            rm_argmax<NR>(re, im, J, lane, &ps, &js);
            double fit = nan, fre = nan, fim = nan;
            if (js >= 0) {
                const double phi = phi0 + (double)js * dphi;
                fit = phi;
                fre = rm_pick<NR>(re, js), fim = rm_pick<NR>(im, js);
                if (js > 0 && js < J - 1) {
                    const double ar = rm_pick<NR>(re, js - 1), ai = rm_pick<NR>(im, js - 1);
                    const double br = rm_pick<NR>(re, js + 1), bi = rm_pick<NR>(im, js + 1);
                    const double pm = ar * ar + ai * ai, pp = br * br + bi * bi;
                    const double d = (pm - ps) + (pp - ps);
                    if (d < 0.0) {
                        const double off = (0.5 * (pm - pp)) / d;
                        fit = phi + off * dphi;
                    }
                }
            } else {
                ps = nan;
            }
            if (lane == 0) {
                a.maps[m] = (double)it, a.maps[a.M + m] = (double)reason, a.maps[2 * a.M + m] = (double)js;
                a.maps[3 * a.M + m] = ps, a.maps[4 * a.M + m] = fit, a.maps[5 * a.M + m] = fre, a.maps[6 * a.M + m] = fim;
            }
            n_it += (u64)it, n_niter += reason == 0, n_level += reason == 1;
        } else if (live) {
            if (lane == 0) {
                a.maps[m] = 0.0, a.maps[a.M + m] = 3.0, a.maps[2 * a.M + m] = -1.0;
                a.maps[3 * a.M + m] = nan, a.maps[4 * a.M + m] = nan, a.maps[5 * a.M + m] = nan, a.maps[6 * a.M + m] = nan;
            }
            n_bad += 1;
        }
        if (STAGE) {  // (without it the waves of a group never wait for each other)
            __syncthreads();  // (wr of the group before has been read)
            if (lane == 0) wr[wave] = good ? 1 : 0;
            __syncthreads();
        }
        rm_store<NR, STAGE>(a.cube, a.M, J, base, Ts, wr, good, re, im);
        if (a.model) rm_store<NR, STAGE>(a.model, a.M, J, base, Ts, wr, good, mre, mim);
    }
    if (lane == 0) {
        if (n_bad) atomicAdd(&a.cnt->bad, n_bad);
        if (n_it) atomicAdd(&a.cnt->iters, n_it);
        if (n_niter) atomicAdd(&a.cnt->by_niter, n_niter);
        if (n_level) atomicAdd(&a.cnt->by_level, n_level);
    }
}

__global__ void rm_clean_stats_kernel(RmClean a, double *__restrict__ stats)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    int C;
    const bool ok = rm_head_ok(a.tables, -1, a.J, &C);
    bool nan_sigma;
    const double L = rm_level(a.threshold, a.nsigma, a.noise, &nan_sigma);
    for (int i = 0; i < GRIDHIP_RM_STATS; ++i) stats[i] = 0.0;
    if (nan_sigma) {
        stats[6] = 1.0;
    } else if (!ok) {
        stats[7] = 1.0;
    } else {
        stats[0] = (double)a.cnt->bad, stats[1] = (double)a.cnt->iters, stats[2] = (double)a.cnt->by_niter;
        stats[3] = (double)a.cnt->by_level, stats[5] = L;
    }
}

bool rm_shape_ok(int64_t C, int64_t J) { return C >= 1 && C <= RM_MAX_C && J >= 1 && J <= RM_MAX_J; }

size_t rm_table_bytes(int64_t C, int64_t J) { return (size_t)GRIDHIP_RM_TABLE_DOUBLES(C, J) * 8; }

int rm_tables_any(gridhip_ctx *ctx, bool dev, int64_t C, int64_t J, const double *lam2, const double *weights, double phi0,
                  double dphi, double fwhm, double *tables)
{
    if (!ctx) return GRIDHIP_EINVAL;
    if (!rm_shape_ok(C, J) || !lam2 || !tables || !isfinite(phi0) || !isfinite(dphi) || !isfinite(fwhm) || !(dphi > 0.0) ||
        !(fwhm > 0.0))
        return fail(ctx, GRIDHIP_EINVAL, "rm_tables: bad argument");
    const size_t cb = (size_t)C * 8, tb = rm_table_bytes(C, J);
    if (outputs_clash({{tables, tb}}, {{lam2, cb}, {weights, cb}}) || overlap(lam2, cb, weights, cb))
        return fail(ctx, GRIDHIP_EINVAL, "rm_tables: arrays overlap");
    GH_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    Staged sg(ctx, dev);
    lam2 = sg.in(lam2, cb), weights = sg.in(weights, cb), tables = sg.out(tables, tb);
    GH_CHECK(sg.status());
    hipLaunchKernelGGL(rm_head_kernel, dim3(1), dim3(64), 0, ctx->stream, (int)C, (int)J, lam2, weights, phi0, dphi, fwhm,
                       tables);
    hipLaunchKernelGGL(rm_fill_kernel, grid_for(ctx, C * J + 4 * J - 2), dim3(256), 0, ctx->stream, (int)C, (int)J, lam2,
                       weights, tables);
    GH_CHECK_HIP(ctx, hipGetLastError());
    return sg.finish();
}

int rmsynth_any(gridhip_ctx *ctx, bool dev, int64_t M, int64_t C, int64_t J, const double *tables, const double *Q,
                const double *U, double *cube, double *stats)
{
    if (!ctx) return GRIDHIP_EINVAL;
    if (M < 1 || !rm_shape_ok(C, J) || !tables || !Q || !U || !cube || !stats || ((uintptr_t)cube & 15))
        return fail(ctx, GRIDHIP_EINVAL, "rmsynth: bad argument");
    const int64_t ndt = (J + RM_TJ - 1) / RM_TJ, nlt = (M + RM_TM - 1) / RM_TM;
    if (M > ((int64_t)1 << 40) || nlt * ndt > 0x7fffffffLL)
        return fail(ctx, GRIDHIP_EUNSUPPORTED, "rmsynth: M above what one launch holds (pass the image in slabs)");
    const size_t tb = rm_table_bytes(C, J), qb = (size_t)C * M * 8, cb = (size_t)J * M * 16;
    if (outputs_clash({{cube, cb}, {stats, 64}}, {{tables, tb}, {Q, qb}, {U, qb}}) || overlap(tables, tb, Q, qb) ||
        overlap(tables, tb, U, qb) || overlap(Q, qb, U, qb))
        return fail(ctx, GRIDHIP_EINVAL, "rmsynth: arrays overlap");
    GH_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    DevBuf cnt;
    GH_CHECK(cnt.alloc(ctx, sizeof(RmCount)));
    Staged sg(ctx, dev);
    tables = sg.in(tables, tb), Q = sg.in(Q, qb), U = sg.in(U, qb);
    cube = sg.inout(cube, cube, cb);  // (invalid tables leave it as it is, in the host form too)
    stats = sg.out(stats, 64);
    GH_CHECK(sg.status());
    hipLaunchKernelGGL(rm_zero_kernel, dim3(1), dim3(64), 0, ctx->stream, cnt.as<RmCount>());
    hipLaunchKernelGGL(rm_synth_kernel, dim3((unsigned)(nlt * ndt)), dim3(RM_THREADS), 0, ctx->stream, M, (int)C, (int)J,
                       (int)ndt, tables, Q, U, reinterpret_cast<double2 *>(cube), cnt.as<RmCount>());
    hipLaunchKernelGGL(rm_synth_stats_kernel, dim3(1), dim3(64), 0, ctx->stream, (int)C, (int)J, tables,
                       (const RmCount *)cnt.as<RmCount>(), stats);
    GH_CHECK_HIP(ctx, hipGetLastError());
    return sg.finish();
}

template <bool STAGE>
void rm_clean_launch(gridhip_ctx *ctx, dim3 grid, const RmClean &a)
{
    const int nr = (a.J + 63) / 64;
    if (nr <= 1)
        hipLaunchKernelGGL((rm_clean_kernel<1, STAGE>), grid, dim3(RM_THREADS), 0, ctx->stream, a);
    else if (nr <= 2)
        hipLaunchKernelGGL((rm_clean_kernel<2, STAGE>), grid, dim3(RM_THREADS), 0, ctx->stream, a);
    else if (nr <= 4)
        hipLaunchKernelGGL((rm_clean_kernel<4, STAGE>), grid, dim3(RM_THREADS), 0, ctx->stream, a);
    else
        hipLaunchKernelGGL((rm_clean_kernel<8, STAGE>), grid, dim3(RM_THREADS), 0, ctx->stream, a);
}

int rmclean_any(gridhip_ctx *ctx, bool dev, int64_t M, int64_t J, const double *tables, double *cube, double *model,
                double gain, double threshold, int64_t niter, double nsigma, const double *noise, int restore, double *maps,
                double *stats)
{
    if (!ctx) return GRIDHIP_EINVAL;
    if (M < 1 || !rm_shape_ok(1, J) || !tables || !cube || !maps || !stats || !isfinite(gain) || !isfinite(threshold) ||
        niter < 0 || !(nsigma >= 0.0 && nsigma < __builtin_inf()) || (nsigma > 0.0 && !noise) ||
        (restore != 0 && restore != 1) || (restore == 1 && !model) || ((uintptr_t)cube & 15) || ((uintptr_t)model & 15))
        return fail(ctx, GRIDHIP_EINVAL, "rmclean: bad argument");
    if (M > ((int64_t)1 << 40)) return fail(ctx, GRIDHIP_EUNSUPPORTED, "rmclean: M above 2^40 (pass the image in slabs)");
    // The table's size follows from its head's C, which the host form reads where it can (host memory); for the overlap
    // rule the smallest table of J depths stands in for a table on the device.
    size_t tb = rm_table_bytes(1, J);
    bool whole = true;
    if (!dev) {
        const double hc = tables[1];
        whole = tables[0] == 1.0 && hc >= 1.0 && hc <= (double)RM_MAX_C && hc == (double)(int64_t)hc && tables[2] == (double)J;
        tb = whole ? rm_table_bytes((int64_t)hc, J) : (size_t)RM_HEAD * 8;  // (a head that does not fit: the kernels see it)
    }
    const size_t cb = (size_t)J * M * 16, mb = (size_t)GRIDHIP_RM_MAPS * M * 8;
    if (nsigma == 0.0) noise = nullptr;  // (not read)
    if (outputs_clash({{cube, cb}, {model, cb}, {maps, mb}, {stats, 64}}, {{tables, tb}, {noise, 8}}) ||
        overlap(tables, tb, noise, 8))
        return fail(ctx, GRIDHIP_EINVAL, "rmclean: arrays overlap");
    GH_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    DevBuf cnt;
    GH_CHECK(cnt.alloc(ctx, sizeof(RmCount)));
    Staged sg(ctx, dev);
    RmClean a;
    a.M = M, a.J = (int)J, a.gain = gain, a.threshold = threshold, a.nsigma = nsigma, a.niter = niter, a.restore = restore;
    a.tables = sg.in(tables, tb);
    a.cube = reinterpret_cast<double2 *>(sg.inout(cube, cube, cb));
    a.model = reinterpret_cast<double2 *>(sg.inout(model, model, cb));
    a.noise = sg.in(noise, 8);
    a.maps = sg.inout(maps, maps, mb);  // (a call that ends early leaves them as they are, in the host form too)
    stats = sg.out(stats, 64);
    a.cnt = cnt.as<RmCount>();
    GH_CHECK(sg.status());
    const int64_t groups = (M + RM_GROUP - 1) / RM_GROUP, most = (int64_t)ctx->num_cu * 20;
    const dim3 grid((unsigned)(groups < most ? groups : most));
    hipLaunchKernelGGL(rm_zero_kernel, dim3(1), dim3(64), 0, ctx->stream, a.cnt);
    if (ctx->img->rm_stage == 1)
        rm_clean_launch<true>(ctx, grid, a);
    else
        rm_clean_launch<false>(ctx, grid, a);
    hipLaunchKernelGGL(rm_clean_stats_kernel, dim3(1), dim3(64), 0, ctx->stream, a, stats);
    GH_CHECK_HIP(ctx, hipGetLastError());
    return sg.finish();
}

}  // namespace

}  // namespace gridhip

using namespace gridhip;

extern "C" {

int gridhip_rm_tables(gridhip_ctx *ctx, int64_t C, int64_t J, const double *lam2, const double *weights, double phi0,
                      double dphi, double fwhm, double *tables)
{
    return rm_tables_any(ctx, false, C, J, lam2, weights, phi0, dphi, fwhm, tables);
}

int gridhip_rm_tables_dev(gridhip_ctx *ctx, int64_t C, int64_t J, const double *lam2, const double *weights, double phi0,
                          double dphi, double fwhm, double *tables)
{
    return rm_tables_any(ctx, true, C, J, lam2, weights, phi0, dphi, fwhm, tables);
}

int gridhip_rmsynth(gridhip_ctx *ctx, int64_t M, int64_t C, int64_t J, const double *tables, const double *Q, const double *U,
                    double *cube, double *stats)
{
    return rmsynth_any(ctx, false, M, C, J, tables, Q, U, cube, stats);
}

int gridhip_rmsynth_dev(gridhip_ctx *ctx, int64_t M, int64_t C, int64_t J, const double *tables, const double *Q,
                        const double *U, double *cube, double *stats)
{
    return rmsynth_any(ctx, true, M, C, J, tables, Q, U, cube, stats);
}

int gridhip_rmclean(gridhip_ctx *ctx, int64_t M, int64_t J, const double *tables, double *cube, double *model, double gain,
                    double threshold, int64_t niter, double nsigma, const double *noise, int restore, double *maps,
                    double *stats)
{
    return rmclean_any(ctx, false, M, J, tables, cube, model, gain, threshold, niter, nsigma, noise, restore, maps, stats);
}

int gridhip_rmclean_dev(gridhip_ctx *ctx, int64_t M, int64_t J, const double *tables, double *cube, double *model, double gain,
                        double threshold, int64_t niter, double nsigma, const double *noise, int restore, double *maps,
                        double *stats)
{
    return rmclean_any(ctx, true, M, J, tables, cube, model, gain, threshold, niter, nsigma, noise, restore, maps, stats);
}

int gridhip_rm_tile(int64_t *out)
{
    if (!out) return GRIDHIP_EINVAL;
    out[0] = RM_TM, out[1] = RM_TJ, out[2] = RM_KC;
    return GRIDHIP_OK;
}

}  // extern "C"
