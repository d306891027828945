// Multi-scale CLEAN (include/gridhip.h, "multi-scale deconvolution"): clean.hip's tile-peak table, on-device stop state
// and two-launch iteration, widened to S scales, and restore.hip's LDS-tiled direct convolution for the set-up.  The walk
// over a tile, the table's reduction and the launch loop are clean_walk.h's, the same code as clean.hip runs.
//
// A component of scale s is the tapered paraboloid m_s (the delta for s = 0) instead of one cell.  The loop keeps one
// residual per scale, R_t = m_t (*) residual (R_0 is the caller's residual itself), and subtracts from each the cross-PSF
// P_{s* t} = m_t (*) m_s* (*) psf of the scale taken, so that every R_t stays the smoothed current residual without ever
// being convolved again.  One call is
//     ms_taps_kernel             the taps of m_1 .. m_{S-1} and the table of pointers to the cross-PSFs and the R_t
//     ms_conv_kernel  x (S (S + 1) / 2 - 1)   the cross-PSFs          (an imager keeps them between calls)
//     ms_conv_kernel  x (S - 1)               the smoothed residuals
//     ms_tile_kernel<false>      builds the S tile tables, one slice of blockIdx.z each
//     ms_pick_kernel<true>       zeroes the state, reduces the S tables, tests the stop rule, chooses the scale, takes the
//                                first component and adds its blob to the model
//     niter x { ms_tile_kernel<true>   slice t subtracts f * P_{s* t} from R_t over the tiles the update region overlaps and
//                                      recomputes their entries of table t in the same pass
//               ms_pick_kernel<false>  the next component }
// so an iteration is two launches and moves S times the bytes of a Hogbom iteration.  Everything the iteration needs - s*,
// k, f, the pointers - lives in the state block on the device; the host reads nothing back, and a launch that finds the
// state stopped returns at its first instruction.  No atomics; contraction is off wherever the header orders a rounding.
#include "common.h"
#include "clean_walk.h"

namespace gridhip {

namespace {

constexpr int MS_TAPS = 63 * 63;                                          // the taps one scale may have (radius 31)
constexpr int MS_PAIRS = MS_MAX_SCALES * (MS_MAX_SCALES + 1) / 2;         // cross-PSFs P_st, s <= t, P_00 the psf itself

__host__ __device__ inline int pair_index(int s, int t) { return s <= t ? t * (t + 1) / 2 + s : s * (s + 1) / 2 + t; }

struct MsState {  // the head of the scratch block
    double peak;        // R_0's current peak (signed); NaN when no cell can be selected
    long long k0;       // its flat index, -1 when none
    long long iters;    // components taken so far
    double flux;        // sum of the f added
    double f;           // gain * (p / q) of the component the next tile kernel subtracts
    long long k;        // its centre
    long long s;        // its scale
    long long stopped;  // every later launch returns
    long long last;     // the scale of the last component taken, -1 when none
    long long n[MS_MAX_SCALES];     // components taken per scale
    const double *P[MS_PAIRS];      // P[pair_index(s, t)]; P[0] is the psf
    double *R[MS_MAX_SCALES];       // the smoothed residuals; R[0] is not used (the residual is a kernel argument)
    double T;                       // the stop level (the _auto forms: the first pick computes it)
    long long reason;               // why the loop stopped (the _auto forms' codes)
};

struct MsScales {  // by value to the kernels: read from the host arrays at call time
    int S;
    int R[MS_MAX_SCALES];     // the radius of m_s: ceil(a_s) - 1 (0 for the delta)
    double a[MS_MAX_SCALES];
    double b[MS_MAX_SCALES];
};

struct MsPointers {  // by value to ms_taps_kernel, which writes them into the state block
    const double *P[MS_PAIRS];
    double *R[MS_MAX_SCALES];
};

// The taps of m_s, s = blockIdx.x + 1: t = max(0, 1 - (dx^2 + dy^2) / a^2) in fp64 with a rounded quotient, summed from
// +0.0 each row in dx order (thread dy + R owns row dy), then the rows in dy order by thread 0, then m = t / sum.
// Block 0 also writes the pointer table.
__global__ void __launch_bounds__(64) ms_taps_kernel(MsScales sc, MsPointers ptr, double *__restrict__ taps, MsState *st)
{
#pragma clang fp contract(off)
    __shared__ double rowsum[64];
    __shared__ double total;
    const int t = threadIdx.x;
    if (blockIdx.x == 0) {
        if (t < MS_PAIRS) st->P[t] = ptr.P[t];
        if (t < MS_MAX_SCALES) st->R[t] = ptr.R[t];
    }
    const int s = blockIdx.x + 1;
    if (s >= sc.S) return;
    const int R = sc.R[s], K = 2 * R + 1;
    const double a2 = sc.a[s] * sc.a[s];
    double *m = taps + (size_t)(s - 1) * MS_TAPS;
    if (t < K) {
        const int dy = t - R;
        double sum = 0.0;
        for (int dx = -R; dx <= R; ++dx) {
            const double r2 = (double)(dx * dx + dy * dy);
            const double v = 1.0 - r2 / a2;
            const double tap = v > 0.0 ? v : 0.0;
            m[t * K + dx + R] = tap;
            sum += tap;
        }
        rowsum[t] = sum;
    }
    __syncthreads();
    if (t == 0) {
        double sum = 0.0;
        for (int r = 0; r < K; ++r) sum += rowsum[r];
        total = sum;
    }
    __syncthreads();
    if (t < K)
        for (int i = 0; i < K; ++i) m[t * K + i] = m[t * K + i] / total;
}

// out = m (*) in: out[y, x] = sum of in[y - dy, x - dx] * m(dy, dx) over |dy|, |dx| <= s, cells outside the image zero, the
// taps dy ascending, then dx ascending, one fused multiply-add each from +0.0.  The tile, the halo staging, the LDS layout
// and the register blocking are restore_kernel's (restore.hip's head explains them); the taps come from the table
// ms_taps_kernel made, staged once per work-group, and a work-group whose staged window holds no non-zero cell stores
// +0.0, which is what the sum gives (the taps are finite).
// grid (ceil(N / RS_TW), ceil(N / RS_TH)); dynamic LDS: restore_lds_bytes(s); stride = staged_stride(s); out is not in.
__global__ void __launch_bounds__(256)
    ms_conv_kernel(int64_t N, const double *__restrict__ in, const double *__restrict__ taps, int s, int stride,
                   double *__restrict__ out)
{
    extern __shared__ __align__(16) double lds[];
    const int t = threadIdx.x, lx = t % RS_LX, ly = t / RS_LX;
    const int64_t x0 = (int64_t)blockIdx.x * RS_TW, y0 = (int64_t)blockIdx.y * RS_TH;
    const int64_t y = y0 + ly, xf = x0 + 8 * lx;  // this thread's row and first cell
    const int rows = RS_TH + 2 * s, cols = RS_TW + 2 * s, K = 2 * s + 1;
    double *wt = lds + (size_t)rows * stride;
    int any = 0;
    for (int i = t; i < rows * cols; i += 256) {
        const int r = i / cols, u = i - r * cols;
        const int64_t gy = y0 - s + r, gx = x0 - s + u;
        double v = 0.0;
        if (gy >= 0 && gy < N && gx >= 0 && gx < N) v = in[gy * N + gx];
        any |= v != 0.0;  // (true for a NaN)
        lds[r * stride + staged_pos(u)] = v;
    }
    any = __syncthreads_or(any);
    double acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.0;
    if (any) {
        for (int i = t; i < K * K; i += 256) wt[i] = taps[i];
        __syncthreads();
        for (int dy = -s; dy <= s; ++dy) {
            const double *mrow = lds + (ly + s - dy) * stride + 9 * lx;  // cell 8 lx + k of the row: mrow[k + k / 8]
            const double *wrow = wt + (dy + s) * K + s;                  // wrow[dx]
            // tap dx of cell j reads cell k = s - dx + j; a chunk of 8 taps keeps 15 cells in registers (restore_kernel)
            double W[15];
            int kb = 2 * s, dx0 = -s;
#pragma unroll
            for (int e = 1; e < 8; ++e) W[e + 7] = mrow[staged_pos(kb + e)];
            for (int c = 0; c < K / 8; ++c, dx0 += 8, kb -= 8) {
#pragma unroll
                for (int e = -7; e <= 0; ++e) W[e + 7] = mrow[staged_pos(kb + e)];
#pragma unroll
                for (int d = 0; d < 8; ++d) {
                    const double w = wrow[dx0 + d];
#pragma unroll
                    for (int j = 0; j < 8; ++j) acc[j] = fma(W[j - d + 7], w, acc[j]);
                }
#pragma unroll
                for (int e = 0; e < 7; ++e) W[e + 8] = W[e];
            }
            for (; dx0 <= s; ++dx0, --kb) {
                const double w = wrow[dx0];
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[j] = fma(mrow[staged_pos(kb + j)], w, acc[j]);
            }
        }
    }
    if (y < N)
        for (int j = 0; j < 8; ++j)
            if (xf + j < N) out[y * N + xf + j] = acc[j];
}

// clean_tile_kernel with a third grid dimension: slice t = blockIdx.z walks R_t and table t (clean_tile_walk,
// clean_walk.h).  SUB = false: grid (ntx, nty, S), the entry of every tile from R_t as it is.  SUB = true: grid (the most
// tiles the update region overlaps, S); slice t subtracts f * P_{s* t}, shifted to the component's centre, over Hogbom's
// update region and recomputes the entries of the tiles it touched in the same pass.  s*, k and f come from the state
// block.  MASK: a cell whose mask byte is 0 is not searched, in any slice - the mask constrains component centres; the
// subtraction does not look at it.
template <bool SUB, bool MASK>
__global__ void __launch_bounds__(256)
    ms_tile_kernel(int64_t N, int64_t border, int64_t patch, int ntx, int ntiles, double *residual,
                   CleanEntry *__restrict__ tables, const MsState *st, const uint8_t *__restrict__ mask)
{
    __shared__ CleanEntry sh[4];
    if (SUB && st->stopped) return;
    const int slice = blockIdx.z;
    double *res = slice == 0 ? residual : st->R[slice];
    const long long k = SUB ? st->k : 0;
    const double f = SUB ? st->f : 0.0;
    const double *psf = SUB ? st->P[pair_index((int)st->s, slice)] : nullptr;
    clean_tile_walk<SUB>(N, border, patch, ntx, k, tables + (size_t)slice * ntiles, sh,
                         OneTermWalk<MASK>{res, psf, 0, f, mask});
}

// One work-group.  Each table's best is that scale's peak p_s at k_s.  Then the head of the next iteration, by thread 0:
// the stop test on scale 0 - nothing to select, out of iterations or |p_0| <= threshold, before anything is subtracted -
// and the choice of s*, the largest |b_s (p_s / q_s)| with q_s = P_ss[c, c], ties to the lowest s, a scale without a
// selectable cell or whose q_s is not positive and finite never; no scale left stops the loop too.  The component
// f = gain * (p / q) at k goes into the state for the next tile kernel, and the whole work-group adds its blob
// f * m_s* to the model (for the delta the one cell, as gridhip_clean adds it).  INIT: the first pick of a call, which starts the
// counters from zero whatever the block held (the pointer table stays).  AUTO: clean_pick_kernel's - the stop level T
// from p_0 of the first pick, the reason codes (no scale left counts as nothing selectable), 16 stats.
template <bool INIT, bool AUTO>
__global__ void __launch_bounds__(1024)
    ms_pick_kernel(int64_t N, int ntiles, const CleanEntry *__restrict__ tables, MsState *st, MsScales sc,
                   const double *__restrict__ taps, double *model, double gain, double threshold, int64_t niter,
                   double *stats, double nsigma, const double *noise, double peak_frac)
{
#pragma clang fp contract(off)
    __shared__ CleanEntry sh[16];
    __shared__ CleanEntry best[MS_MAX_SCALES];
    __shared__ double sh_f, sh_r;
    __shared__ long long sh_k;
    __shared__ int sh_s;
    if (!INIT && st->stopped) return;
    for (int s = 0; s < sc.S; ++s) {
        double bv;
        long long bk;
        table_best(tables + (size_t)s * ntiles, ntiles, bv, bk, sh);
        if (threadIdx.x == 0) best[s] = {bv, bk};
        __syncthreads();  // (sh is free for the next scale)
    }
    if (threadIdx.x == 0) {
        long long iters = INIT ? 0 : st->iters, last = INIT ? -1 : st->last;
        double flux = INIT ? 0.0 : st->flux;
        long long n[MS_MAX_SCALES];
        for (int s = 0; s < MS_MAX_SCALES; ++s) n[s] = INIT ? 0 : st->n[s];
        const long long k0 = best[0].k;
        const double peak = k0 < 0 ? __builtin_nan("") : best[0].v;
        bool bad = false;
        if (AUTO) threshold = INIT ? stop_level(threshold, nsigma, noise, peak_frac, peak, &bad) : st->T;
        bool stop = bad || k0 < 0 || iters >= niter || !(fabs(best[0].v) > threshold);
        long long reason = !stop ? 0 : bad ? 3 : k0 < 0 ? 2 : !(fabs(best[0].v) > threshold) ? 1 : 0;
        int pick = -1;
        if (!stop) {
            const int64_t c = N / 2;
            double top = 0.0, q_pick = 1.0;
            for (int s = 0; s < sc.S; ++s) {
                if (best[s].k < 0) continue;
                const double q = st->P[pair_index(s, s)][c * N + c];
                if (!(q > 0.0 && q < __builtin_inf())) continue;
                const double r = best[s].v / q;
                const double v = fabs(sc.b[s] * r);
                if (pick < 0 || v > top) pick = s, top = v, q_pick = q;
            }
            if (pick < 0) {
                stop = true;
                reason = 2;
            } else {
                const double r = best[pick].v / q_pick;
                const double f = gain * r;
                sh_r = r;
                flux += f;
                iters += 1;
                n[pick] += 1;
                last = pick;
                st->f = f;
                st->k = best[pick].k;
                st->s = pick;
                sh_f = f;
                sh_k = best[pick].k;
            }
        }
        sh_s = pick;
        st->peak = peak;
        st->k0 = k0;
        st->iters = iters;
        st->flux = flux;
        st->last = last;
        for (int s = 0; s < MS_MAX_SCALES; ++s) st->n[s] = n[s];
        st->stopped = stop ? 1 : 0;
        if (stats) {
            stats[0] = (double)iters;
            stats[1] = peak;
            stats[2] = (double)k0;
            stats[3] = (double)last;
            stats[4] = flux;
            stats[5] = 0.0;
            for (int s = 0; s < MS_MAX_SCALES; ++s) stats[6 + s] = (double)n[s];
        }
        if (AUTO) {
            st->T = threshold;
            st->reason = reason;
            if (stats) {
                if (INIT) stats[12] = threshold, stats[14] = peak, stats[15] = 0.0;
                stats[13] = (double)reason;
            }
        }
    }
    __syncthreads();
    const int s = sh_s;
    if (s < 0) return;
    const double f = sh_f;
    const int64_t k = sh_k;
    if (s == 0) {
        // gridhip_clean's pick kernel is compiled with contraction on and adds gain * p to the model cell in one fused
        // step; the delta component does the same, so that the delta scale alone gives gridhip_clean's bits
        if (threadIdx.x == 0) model[k] = fma(gain, sh_r, model[k]);
        return;
    }
    const int R = sc.R[s], K = 2 * R + 1;
    const double *m = taps + (size_t)(s - 1) * MS_TAPS;
    const int64_t y = k / N, x = k % N;
    for (int i = threadIdx.x; i < K * K; i += blockDim.x) {
        const int iy = i / K;
        const int64_t yy = y + iy - R, xx = x + (i - iy * K) - R;
        if (yy < 0 || yy >= N || xx < 0 || xx >= N) continue;
        const double add = f * m[i];
        model[yy * N + xx] = model[yy * N + xx] + add;
    }
}

// the sizes of the scratch block's parts, in bytes
struct MsLayout {
    size_t state, tables, taps, image, total;
    int nimages;
};
MsLayout layout(int64_t N, int64_t S)
{
    MsLayout l;
    l.state = (sizeof(MsState) + 255) & ~(size_t)255;
    l.tables = ((size_t)S * clean_tiles(N).ntiles * sizeof(CleanEntry) + 255) & ~(size_t)255;
    l.taps = ((size_t)(S - 1) * MS_TAPS * sizeof(double) + 255) & ~(size_t)255;
    l.image = ((size_t)N * N * sizeof(double) + 255) & ~(size_t)255;
    l.nimages = (int)((S - 1) + S * (S + 1) / 2 - 1);
    l.total = l.state + l.tables + l.taps + (size_t)l.nimages * l.image;
    return l;
}

struct MsLaunch {  // what the tile and pick launches of one call take
    gridhip_ctx *ctx;
    int64_t N, border, patch;
    CleanTiles t;  // (all and part with S slices)
    double *residual;
    CleanEntry *tables;
    MsState *st;
    MsScales sc;
    const double *taps;
    double *model;
    double gain, threshold;
    int64_t niter;
    double *stats;
    CleanAuto au;
};

template <bool MASK, bool AUTO>
void ms_launch(const MsLaunch &a)
{
    hipStream_t q = a.ctx->stream;
    const auto tile = [&](auto sub, const dim3 &grid) {
        hipLaunchKernelGGL((ms_tile_kernel<decltype(sub)::value, MASK>), grid, dim3(256), 0, q, a.N, a.border, a.patch,
                           a.t.ntx, a.t.ntiles, a.residual, a.tables, (const MsState *)a.st, a.au.mask);
    };
    const auto pick = [&](auto init) {
        hipLaunchKernelGGL((ms_pick_kernel<decltype(init)::value, AUTO>), dim3(1), dim3(1024), 0, q, a.N, a.t.ntiles,
                           (const CleanEntry *)a.tables, a.st, a.sc, a.taps, a.model, a.gain, a.threshold, a.niter,
                           a.stats, a.au.nsigma, a.au.noise, a.au.peak_frac);
    };
    clean_launch_loop(
        a.niter, [&] { tile(std::false_type{}, a.t.all); }, [&] { pick(std::true_type{}); },
        [&] { tile(std::true_type{}, a.t.part); }, [&] { pick(std::false_type{}); });
}

int conv(gridhip_ctx *ctx, int64_t N, const double *in, const double *taps, int s, double *out)
{
    const dim3 grid((unsigned)((N + RS_TW - 1) / RS_TW), (unsigned)((N + RS_TH - 1) / RS_TH));
    hipLaunchKernelGGL(ms_conv_kernel, grid, dim3(256), restore_lds_bytes(s), ctx->stream, N, in, taps, s, staged_stride(s),
                       out);
    GH_CHECK_HIP(ctx, hipGetLastError());
    return GRIDHIP_OK;
}

}  // namespace

int msclean_check(gridhip_ctx *ctx, int64_t N, const double *psf, const double *residual, const double *model, int64_t S,
                  const double *scales, const double *bias, double gain, double threshold, int64_t niter, int64_t border,
                  int64_t patch)
{
    GH_CHECK(clean_check(ctx, N, psf, residual, model, gain, threshold, niter, border, patch));
    if (S < 1 || S > MS_MAX_SCALES || !scales || !bias) return fail(ctx, GRIDHIP_EINVAL, "msclean: bad scale list");
    if (scales[0] != 0.0) return fail(ctx, GRIDHIP_EINVAL, "msclean: the first scale must be 0");
    for (int64_t s = 0; s < S; ++s) {
        if (s > 0 && !(scales[s] > scales[s - 1]))
            return fail(ctx, GRIDHIP_EINVAL, "msclean: the scales must be strictly increasing");
        if (!(bias[s] > 0.0 && bias[s] < __builtin_inf()))
            return fail(ctx, GRIDHIP_EINVAL, "msclean: a bias must be finite and positive");
    }
    if (scales[S - 1] > MS_MAX_SCALE) return fail(ctx, GRIDHIP_EUNSUPPORTED, "msclean: a scale above 32 cells");
    return GRIDHIP_OK;
}

size_t msclean_scratch_bytes(int64_t N, int64_t S) { return layout(N, S).total; }

int msclean_run(gridhip_ctx *ctx, int64_t N, const double *psf, double *residual, double *model, int64_t S,
                const double *scales, const double *bias, double gain, double threshold, int64_t niter, int64_t border,
                int64_t patch, double *stats, void *scratch, bool setup, const CleanAuto &au)
{
    const MsLayout l = layout(N, S);
    char *base = reinterpret_cast<char *>(scratch);
    MsState *st = reinterpret_cast<MsState *>(base);
    CleanEntry *tables = reinterpret_cast<CleanEntry *>(base + l.state);
    double *taps = reinterpret_cast<double *>(base + l.state + l.tables);
    char *images = base + l.state + l.tables + l.taps;
    MsScales sc = {};
    sc.S = (int)S;
    for (int s = 0; s < (int)S; ++s) {
        sc.a[s] = scales[s];
        sc.b[s] = bias[s];
        sc.R[s] = s == 0 ? 0 : (int)ceil(scales[s]) - 1;
    }
    // the images: R_1 .. R_{S-1}, then the cross-PSFs in pair_index order
    MsPointers ptr = {};
    int next = 0;
    for (int s = 1; s < (int)S; ++s) ptr.R[s] = reinterpret_cast<double *>(images + (size_t)next++ * l.image);
    ptr.P[0] = psf;
    for (int t = 1; t < (int)S; ++t)
        for (int s = 0; s <= t; ++s) ptr.P[pair_index(s, t)] = reinterpret_cast<double *>(images + (size_t)next++ * l.image);
    if (S > 1 && !ctx->img->msconv_lds_raised) {  // (more than 64 KB of LDS only once the function is told so)
        GH_CHECK_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(ms_conv_kernel),
                                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)restore_lds_bytes(31)));
        ctx->img->msconv_lds_raised = true;
    }
    if (setup) {
        hipLaunchKernelGGL(ms_taps_kernel, dim3((unsigned)(S > 1 ? S - 1 : 1)), dim3(64), 0, ctx->stream, sc, ptr, taps, st);
        GH_CHECK_HIP(ctx, hipGetLastError());
        // P_0t = m_t (*) psf, then P_st = m_t (*) P_0s for 1 <= s <= t
        for (int t = 1; t < (int)S; ++t)
            GH_CHECK(conv(ctx, N, psf, taps + (size_t)(t - 1) * MS_TAPS, sc.R[t], const_cast<double *>(ptr.P[pair_index(0, t)])));
        for (int t = 1; t < (int)S; ++t)
            for (int s = 1; s <= t; ++s)
                GH_CHECK(conv(ctx, N, ptr.P[pair_index(0, s)], taps + (size_t)(t - 1) * MS_TAPS, sc.R[t],
                              const_cast<double *>(ptr.P[pair_index(s, t)])));
    }
    for (int t = 1; t < (int)S; ++t) GH_CHECK(conv(ctx, N, residual, taps + (size_t)(t - 1) * MS_TAPS, sc.R[t], ptr.R[t]));

    CleanTiles t = clean_tiles(N, patch);
    t.all.z = t.part.z = (unsigned)S;
    const MsLaunch go = {ctx, N, border, patch, t, residual, tables, st, sc, taps, model, gain, threshold, niter, stats, au};
    if (!au.on)
        ms_launch<false, false>(go);
    else if (au.mask)
        ms_launch<true, true>(go);
    else
        ms_launch<false, true>(go);
    GH_CHECK_HIP(ctx, hipGetLastError());
    return GRIDHIP_OK;
}

}  // namespace gridhip

using namespace gridhip;

namespace {

int msclean_any(gridhip_ctx *ctx, bool dev, int64_t N, const double *psf, double *residual, double *model, int64_t S,
                const double *scales, const double *bias, double gain, double threshold, int64_t niter, int64_t border,
                int64_t patch, double *stats, CleanAuto au = CleanAuto{})
{
    if (!ctx) return GRIDHIP_EINVAL;
    GH_CHECK(msclean_check(ctx, N, psf, residual, model, S, scales, bias, gain, threshold, niter, border, patch));
    if (au.on) GH_CHECK(clean_auto_check(ctx, N, residual, model, au.mask, au.nsigma, au.noise, au.peak_frac));
    GH_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    DevBuf scratch;
    GH_CHECK(scratch.alloc(ctx, msclean_scratch_bytes(N, S)));
    const size_t bytes = (size_t)N * N * 8;
    Staged st(ctx, dev);
    psf = st.in(psf, bytes), residual = st.inout(residual, residual, bytes), model = st.inout(model, model, bytes);
    stats = st.out(stats, au.on ? 128 : 96), au.mask = st.in(au.mask, bytes / 8);
    if (au.nsigma > 0.0) au.noise = st.in(au.noise, 8);
    GH_CHECK(st.status());
    GH_CHECK(msclean_run(ctx, N, psf, residual, model, S, scales, bias, gain, threshold, niter, border, patch, stats,
                         scratch.p, true, au));
    return st.finish();
}

}  // namespace

extern "C" {

int gridhip_msclean(gridhip_ctx *ctx, int64_t N, const double *psf, double *residual, double *model, int64_t S,
                    const double *scales, const double *bias, double gain, double threshold, int64_t niter, int64_t border,
                    int64_t patch, double *stats)
{
    return msclean_any(ctx, false, N, psf, residual, model, S, scales, bias, gain, threshold, niter, border, patch, stats);
}

int gridhip_msclean_dev(gridhip_ctx *ctx, int64_t N, const double *psf, double *residual, double *model, int64_t S,
                        const double *scales, const double *bias, double gain, double threshold, int64_t niter,
                        int64_t border, int64_t patch, double *stats)
{
    return msclean_any(ctx, true, N, psf, residual, model, S, scales, bias, gain, threshold, niter, border, patch, stats);
}

int gridhip_msclean_auto(gridhip_ctx *ctx, int64_t N, const double *psf, double *residual, double *model, int64_t S,
                         const double *scales, const double *bias, double gain, double threshold, int64_t niter,
                         int64_t border, int64_t patch, const uint8_t *mask, double nsigma, const double *noise,
                         double peak_frac, double *stats)
{
    return msclean_any(ctx, false, N, psf, residual, model, S, scales, bias, gain, threshold, niter, border, patch, stats,
                       CleanAuto{mask, nsigma, noise, peak_frac, true});
}

int gridhip_msclean_auto_dev(gridhip_ctx *ctx, int64_t N, const double *psf, double *residual, double *model, int64_t S,
                             const double *scales, const double *bias, double gain, double threshold, int64_t niter,
                             int64_t border, int64_t patch, const uint8_t *mask, double nsigma, const double *noise,
                             double peak_frac, double *stats)
{
    return msclean_any(ctx, true, N, psf, residual, model, S, scales, bias, gain, threshold, niter, border, patch, stats,
                       CleanAuto{mask, nsigma, noise, peak_frac, true});
}

}  // extern "C"
