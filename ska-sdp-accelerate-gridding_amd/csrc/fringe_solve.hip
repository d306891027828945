// The antenna fit of the delay-like calibrations (include/gridhip.h, gridhip_fringe_solve): antenna delays, rates - or
// whatever a module's second axis holds - and phasors from the rows of `peaks` of a search.  fringe_solve.h declares what
// the fit drivers use of it.
//
//     gridhip_fringe_solve    fr_solve_kernel (one work-group per interval), fr_solve_stats_kernel
//     a fit driver            [fr_init_sol_kernel]; per round, behind its search, the two above
// Nothing is read back and the stop test of the solve is inside its kernel, so the _dev form is a fixed chain of launches.
//
// THE SOLVE KERNEL.  One work-group per interval; an antenna belongs to one thread.  The baselines pass through LDS twice
// in chunks of 256, once to count and once to fill, which leaves every antenna the list of its used baselines in ascending
// order in scratch; a Jacobi sweep reads only an antenna's own list, in that order: no floating-point atomic.
#include "delay_arith.h"
#include "fringe_solve.h"
#include "imaging.h"

#pragma clang fp contract(off)

namespace gridhip {

namespace {

constexpr int FR_THREADS = 256;
constexpr int FR_ROW = DL_ROW;
constexpr int FR_MAX_A = GRIDHIP_FRINGE_MAX_ANTENNAS;
constexpr int FR_NA = FR_MAX_A / FR_THREADS;  // antennas of a thread

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
        const bool use = row[10] == 0.0 && row[8] >= a.min_count && coh2 >= a.min_coh2 && coh2 > 0.0 && dl_finite(coh2) &&
                         dl_finite(row[3]) && dl_finite(row[4]) && dl_finite(row[5]) && dl_finite(row[6]) && p >= 0 && p < A &&
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
            if (m2 > 0.0 && dl_finite(m2)) {
                const double sq = sqrt(m2);
                g1 = make_double2(num.x / sq, num.y / sq);
            }
            if (it & 1) {
                t1 = 0.5 * (t1 + xt[s]), r1 = 0.5 * (r1 + xr[s]);
                const double2 av = make_double2(0.5 * (g1.x + hs[s].x), 0.5 * (g1.y + hs[s].y));
                const double n2 = av.x * av.x + av.y * av.y;
                if (n2 > 0.0 && dl_finite(n2)) {
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
            g1 = s == a.refant ? make_double2(1.0, 0.0) : dl_mulc(g1, refh);
        }
        double *so = a.sol + ((int64_t)i * A + s) * 4;
        so[0] = so[0] + t1, so[1] = so[1] + r1;
        const double2 g = dl_mul(make_double2(so[2], so[3]), g1);
        const double m2 = g.x * g.x + g.y * g.y;
        if (m2 > 0.0 && dl_finite(m2)) {
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

int fr_solve_any(gridhip_ctx *ctx, bool dev, int64_t B, int64_t I, int64_t A, const int64_t *a1, const int64_t *a2,
                 const double *peaks, double min_count, double min_coh2, int64_t refant, int64_t niter, double tol,
                 double *sol, double *info, double *stats)
{
    if (!ctx) return GRIDHIP_EINVAL;
    if (!fr_solve_args_ok(B, I, A, min_count, min_coh2, refant, niter, tol) || !a1 || !a2 || !peaks || !sol || !info || !stats)
        return fail(ctx, GRIDHIP_EINVAL, "fringe_solve: bad argument");
    if (!dl_cube_fits(B, I, A)) return fail(ctx, GRIDHIP_EUNSUPPORTED, "fringe_solve: B above 2^24, I above 2^20 or A above 1024");
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

}  // namespace

bool fr_solve_args_ok(int64_t B, int64_t I, int64_t A, double min_count, double min_coh2, int64_t refant, int64_t niter,
                      double tol)
{
    return B >= 1 && I >= 1 && A >= 2 && min_count >= 0.0 && isfinite(min_count) && min_coh2 >= 0.0 && isfinite(min_coh2) &&
           refant < A && niter >= 0 && niter <= GRIDHIP_FRINGE_MAX_ITER && tol >= 0.0 && isfinite(tol);
}

void fr_solve_launch(gridhip_ctx *ctx, const FrSolve &a, double *stats)
{
    hipLaunchKernelGGL(fr_solve_kernel, dim3((unsigned)a.I), dim3(FR_THREADS), 0, ctx->stream, a);
    hipLaunchKernelGGL(fr_solve_stats_kernel, dim3(1), dim3(64), 0, ctx->stream, a, stats);
}

void fr_init_sol_launch(gridhip_ctx *ctx, int64_t n, double *sol)
{
    hipLaunchKernelGGL(fr_init_sol_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, n, sol);
}

}  // namespace gridhip

using namespace gridhip;

extern "C" {

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

}  // extern "C"
