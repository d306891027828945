// Time-frequency flagging (include/gridhip.h, "time-frequency flagging"): SumThreshold over a dense cube of B baselines x
// T time steps x F channels, then the scale-invariant rank (SIR) operator - the flagging that sees interference no single
// sample shows: a burst over a few time steps, a line in one channel.
//
// The front pass (the amplitude key and the baseline code of every sample) and the per-baseline lower median and MAD are
// flag.hip's, shared through imaging.h: flag_front with the cube's group rule, flag_select with sigma_only.  One call is
//     flag_front                          init + front: the classes 1 and 3, the 8-byte key of a, the baseline code; the
//                                         byte code of every sample goes to c8, the call's own array of n bytes
//     niter x { flag_select               32 launches: n_b, med_b, MAD_b of every baseline, chi_0 into baseline_stats
//               K x st_stage_kernel<k>    stage k, both directions in one launch }
//     (niter = 0: flag_select's two launches for the counts)
//     st_sir_fwd_kernel, st_sir_bwd_kernel    along frequency when eta_f > 0, then along time when eta_t > 0
//     st_final_kernel                     wt_out, flags_out, the 8 stats
// 3 + niter (32 + K) + 2 (eta_f > 0) + 2 (eta_t > 0) launches (5 + ... for niter = 0) whatever the data hold.
//
// THE STAGE KERNEL.  A work-group of 256 threads owns a tile of ST_TILE_T x ST_TILE_F samples of one baseline (work-groups
// stride over the tiles).  Per direction it stages x = a - med (or +0.0) and c = 1 (or 0) of the tile and a halo of M - 1
// samples either side along the direction in LDS - [tile_t][tile_f + 2 (M - 1)] along frequency, [tile_t + 2 (M - 1)]
// [tile_f] along time, consecutive threads at consecutive f in both, so every global and every LDS access is along f
// whatever the cube's order - and builds S^(M) and C^(M) by the doubling tree S_j += S_{j+m} in place (every thread reads
// its cells' two operands, a barrier, every thread writes).  The tree of a window that lies inside the row reads cells of
// the row only, so its additions are the header's, in the header's order.  Window j is hit when it lies inside the row
// and S_j > chi * C_j; the sliding OR of the hits over [i - M + 1, i] is the same doubling, backwards, over the array c
// has left.  The hits of the tile's own samples are OR-ed over both directions in a small array, and only then are the
// codes of the tile written: 12 B of LDS per staged cell, 60.7 KB at M = 64 (dynamic, sized by the stage) plus 1 KB.
// Codes are updated in place: a reader takes "code 0 or this stage's own code" for a participant, so both directions of
// every tile see the participants as the previous stage left them, whichever work-group has written first.
// A baseline that is not thresholded (n_b < min_count, sigma_b == 0) is skipped by its work-groups.
//
// THE SIR KERNELS.  One wave per row (along frequency: a row is contiguous; along time: strided), 64 samples at a time
// with the running values carried from chunk to chunk: forward the scan P and the running minimum of P_i, i <= x, both
// kept per sample (16 B); backward the running maximum of P_j, j > x, compared at once.  int64 throughout.
// The stop test is flag.hip's: the stage kernels of round r count what they flag in clipped[r], and every launch of round
// r + 1 returns at once when that is zero.
// Determinism: counts, order statistics, integer sums and a fixed tree of rounded additions (contraction off); no
// floating-point atomic.
#include "common.h"
#include "imaging.h"

namespace gridhip {

namespace {

typedef unsigned long long u64;
typedef unsigned int u32;
typedef long long i64;

constexpr int ST_THREADS = 256;
constexpr int ST_TILE = ST_TILE_T * ST_TILE_F;
static_assert(ST_TILE_T == 32 && ST_TILE_F == 32 && ST_TILE % ST_THREADS == 0, "the stage kernel's index arithmetic");
constexpr i64 SIR_ONE = (i64)1 << 20;

struct Cube {
    int64_t B, T, F;
    int64_t sb, st;  // the strides of b and t in samples (f: 1)
};

template <int K>
struct Stage {
    static constexpr int M = 1 << K, H = M - 1, LD = 32 + 2 * H, CELLS = 32 * LD, PER = (CELLS + ST_THREADS - 1) / ST_THREADS;
    static constexpr size_t LDS = (size_t)CELLS * 12;
};

// Stage K of round `round` (the header's "a stage").  dyn: CELLS doubles, then CELLS ints.
template <int K>
__global__ void __launch_bounds__(ST_THREADS)
    st_stage_kernel(Cube q, int round, double level, int64_t min_count, const u64 *__restrict__ keys, u32 *__restrict__ codes,
                    uint8_t *c8, const FlagGroup *__restrict__ gs, FlagState *st)
{
#pragma clang fp contract(off)
    constexpr int M = Stage<K>::M, H = Stage<K>::H, LD = Stage<K>::LD, CELLS = Stage<K>::CELLS, PER = Stage<K>::PER;
    extern __shared__ double st_lds[];
    __shared__ unsigned char tile_hit[ST_TILE];
    if (flag_stopped(st, round)) return;
    double *S = st_lds;
    int *Cn = reinterpret_cast<int *>(st_lds + CELLS);
    const int tid = threadIdx.x;
    const uint8_t own = (uint8_t)(16 + 8 * round + K);
    const int64_t ntt = (q.T + ST_TILE_T - 1) / ST_TILE_T, ntf = (q.F + ST_TILE_F - 1) / ST_TILE_F;
    const int64_t per_b = ntt * ntf, tiles = q.B * per_b;
    u32 count = 0u;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t b = tile / per_b, rem = tile - b * per_b;
        const int64_t t0 = (rem / ntf) * ST_TILE_T, f0 = (rem % ntf) * ST_TILE_F;
        const double med = gs[b].med, sigma = 1.4826 * gs[b].mad;
        if ((int64_t)gs[b].n < min_count || !(sigma != 0.0)) continue;  // (the same for every thread)
        const double chi = level * sigma;
        const int64_t kb = b * q.sb;
        for (int j = tid; j < ST_TILE; j += ST_THREADS) tile_hit[j] = 0;
        for (int dir = 0; dir < 2; ++dir) {
            const int64_t L = dir ? q.T : q.F;
            if ((int64_t)M > L) continue;
            const int step = dir ? ST_TILE_F : 1;  // the distance in LDS of neighbours along the direction
            __syncthreads();  // (tile_hit zeroed; the other direction has finished with the arrays)
            // cell idx: along frequency [line = t][pos], along time [pos][line = f]; pos counts from the halo's start
#pragma unroll
            for (int i = 0; i < PER; ++i) {
                const int idx = tid + i * ST_THREADS;
                if (idx >= CELLS) continue;
                const int pos = dir ? idx / ST_TILE_F : idx % LD, line = dir ? idx % ST_TILE_F : idx / LD;
                const int64_t t = dir ? t0 - H + pos : t0 + line, f = dir ? f0 + line : f0 - H + pos;
                double x = 0.0;
                int c = 0;
                if (t >= 0 && t < q.T && f >= 0 && f < q.F) {
                    const int64_t k = kb + t * q.st + f;
                    const uint8_t code = c8[k];
                    if (code == 0 || code == own) {
                        x = __builtin_bit_cast(double, keys[k]) - med;
                        c = 1;
                    }
                }
                S[idx] = x;
                Cn[idx] = c;
            }
            __syncthreads();
            // the tree: S^(2m)_j = S^(m)_j + S^(m)_{j+m}
#pragma unroll
            for (int m = 1; m < M; m <<= 1) {
                double rs[PER];
                int rc[PER];
#pragma unroll
                for (int i = 0; i < PER; ++i) {
                    const int idx = tid + i * ST_THREADS;
                    const int pos = dir ? idx / ST_TILE_F : idx % LD;
                    const bool ok = idx < CELLS && pos + m < LD;
                    rs[i] = ok ? S[idx] + S[idx + m * step] : 0.0;
                    rc[i] = ok ? Cn[idx] + Cn[idx + m * step] : 0;
                }
                __syncthreads();
#pragma unroll
                for (int i = 0; i < PER; ++i) {
                    const int idx = tid + i * ST_THREADS;
                    const int pos = dir ? idx / ST_TILE_F : idx % LD;
                    if (idx < CELLS && pos + m < LD) S[idx] = rs[i], Cn[idx] = rc[i];
                }
                __syncthreads();
            }
            // the windows that are hit, into Cn (a thread reads and writes its own cells)
            const int64_t j0 = (dir ? t0 : f0) - H;  // the row position of pos 0
#pragma unroll
            for (int i = 0; i < PER; ++i) {
                const int idx = tid + i * ST_THREADS;
                if (idx >= CELLS) continue;
                const int pos = dir ? idx / ST_TILE_F : idx % LD;
                const int64_t j = j0 + pos;
                const int c = Cn[idx];
                const bool valid = pos + M <= LD && j >= 0 && j <= L - M;
                Cn[idx] = (valid && c > 0 && S[idx] > chi * (double)c) ? 1 : 0;
            }
            __syncthreads();
            // sample i is hit when a window in [i - M + 1, i] is: the sliding OR by the same doubling
#pragma unroll
            for (int m = 1; m < M; m <<= 1) {
                int rc[PER];
#pragma unroll
                for (int i = 0; i < PER; ++i) {
                    const int idx = tid + i * ST_THREADS;
                    const int pos = dir ? idx / ST_TILE_F : idx % LD;
                    rc[i] = idx < CELLS ? (Cn[idx] | (pos >= m ? Cn[idx - m * step] : 0)) : 0;
                }
                __syncthreads();
#pragma unroll
                for (int i = 0; i < PER; ++i) {
                    const int idx = tid + i * ST_THREADS;
                    if (idx < CELLS) Cn[idx] = rc[i];
                }
                __syncthreads();
            }
            // the tile's own samples (each by one thread)
#pragma unroll
            for (int i = 0; i < PER; ++i) {
                const int idx = tid + i * ST_THREADS;
                if (idx >= CELLS) continue;
                const int pos = dir ? idx / ST_TILE_F : idx % LD, line = dir ? idx % ST_TILE_F : idx / LD;
                if (pos < H || pos >= H + 32) continue;
                const int cell = dir ? (pos - H) * ST_TILE_F + line : line * ST_TILE_F + (pos - H);
                if (Cn[idx]) tile_hit[cell] = 1;
            }
        }
        __syncthreads();
        for (int cell = tid; cell < ST_TILE; cell += ST_THREADS) {
            const int64_t t = t0 + cell / ST_TILE_F, f = f0 + cell % ST_TILE_F;
            if (!tile_hit[cell] || t >= q.T || f >= q.F) continue;
            const int64_t k = kb + t * q.st + f;
            if (c8[k] != 0) continue;
            c8[k] = own;
            codes[k] = FLAG_DEAD;
            count += 1u;
        }
        __syncthreads();  // (before tile_hit is zeroed for the next tile)
    }
    flag_wave_count(count, &st->clipped[round]);
}

// the SIR weight of a code: q for what is flagged, q - 2^20 for a kept sample, 0 for a cell flagged on input
__device__ __forceinline__ i64 sir_weight(uint8_t code, i64 qq) { return code == 1 ? 0 : code == 0 ? qq - SIR_ONE : qq; }

// Row r of the direction: along frequency r = b T + t, along time r = b F + f.  *base: its first sample; the return value
// is the distance of its samples.
__device__ __forceinline__ int64_t sir_row(const Cube &q, int dir, int64_t r, int64_t *base)
{
    if (dir == 0) {
        *base = (r / q.T) * q.sb + (r % q.T) * q.st;
        return 1;
    }
    *base = (r / q.F) * q.sb + (r % q.F);
    return q.st;
}

// Forward: per sample x of a row P_{x+1} (pn) and min_{i <= x} P_i (pmin).  One wave per row, 64 samples at a time.
__global__ void __launch_bounds__(ST_THREADS)
    st_sir_fwd_kernel(Cube q, int dir, i64 qq, const uint8_t *__restrict__ c8, i64 *__restrict__ pn, i64 *__restrict__ pmin)
{
    const int lane = threadIdx.x & 63;
    const int64_t rows = dir ? q.B * q.F : q.B * q.T, L = dir ? q.T : q.F;
    const int64_t w0 = ((int64_t)blockIdx.x * ST_THREADS + threadIdx.x) >> 6, nw = ((int64_t)gridDim.x * ST_THREADS) >> 6;
    for (int64_t r = w0; r < rows; r += nw) {
        int64_t base;
        const int64_t d = sir_row(q, dir, r, &base);
        i64 carry_p = 0, carry_min = 0x7fffffffffffffffLL;
        for (int64_t x0 = 0; x0 < L; x0 += 64) {
            const int64_t x = x0 + lane, k = base + x * d;
            const bool valid = x < L;
            const i64 w = valid ? sir_weight(c8[k], qq) : 0;
            i64 inc = w;
            for (int o = 1; o < 64; o <<= 1) {
                const i64 v = __shfl_up(inc, o);
                if (lane >= o) inc += v;
            }
            const i64 p_next = carry_p + inc;
            i64 mn = p_next - w;  // P_x
            for (int o = 1; o < 64; o <<= 1) {
                const i64 v = __shfl_up(mn, o);
                if (lane >= o && v < mn) mn = v;
            }
            if (carry_min < mn) mn = carry_min;
            if (valid) pn[k] = p_next, pmin[k] = mn;
            carry_p = __shfl(p_next, 63);
            carry_min = __shfl(mn, 63);
        }
    }
}

// Backward: a sample of code 0 whose max_{j > x} P_j - min_{i <= x} P_i >= 0 gets the code 8.
__global__ void __launch_bounds__(ST_THREADS)
    st_sir_bwd_kernel(Cube q, int dir, uint8_t *c8, const i64 *__restrict__ pn, const i64 *__restrict__ pmin, FlagState *st)
{
    const int lane = threadIdx.x & 63;
    const int64_t rows = dir ? q.B * q.F : q.B * q.T, L = dir ? q.T : q.F;
    const int64_t w0 = ((int64_t)blockIdx.x * ST_THREADS + threadIdx.x) >> 6, nw = ((int64_t)gridDim.x * ST_THREADS) >> 6;
    const i64 lowest = -0x7fffffffffffffffLL - 1;
    u32 count = 0u;
    for (int64_t r = w0; r < rows; r += nw) {
        int64_t base;
        const int64_t d = sir_row(q, dir, r, &base);
        i64 carry_max = lowest;
        for (int64_t x0 = ((L - 1) / 64) * 64; x0 >= 0; x0 -= 64) {
            const int64_t x = x0 + lane, k = base + x * d;
            const bool valid = x < L;
            i64 mx = valid ? pn[k] : lowest;
            for (int o = 1; o < 64; o <<= 1) {
                const i64 v = __shfl_down(mx, o);
                if (lane + o < 64 && v > mx) mx = v;
            }
            if (carry_max > mx) mx = carry_max;
            if (valid && c8[k] == 0 && mx - pmin[k] >= 0) {
                c8[k] = 8;
                count += 1u;
            }
            carry_max = __shfl(mx, 0);
        }
    }
    flag_wave_count(count, &st->sir);
}

// wt_out = the data weight (1 without data weights) of a kept sample, else +0.0 (wt_out may be wt_in: element k is read
// before it is written, by the same lane); the codes; the first thread writes the 8 stats.
__global__ void __launch_bounds__(256)
    st_final_kernel(int64_t n, int niter, const uint8_t *__restrict__ c8, const double *wt_in, double *wt_out,
                    uint8_t *__restrict__ flags, const FlagState *st, double *__restrict__ stats)
{
    const int64_t k0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, step = (int64_t)gridDim.x * blockDim.x;
    for (int64_t k = k0; k < n; k += step) {
        const double s = wt_in ? wt_in[k] : 1.0;
        const uint8_t c = c8[k];
        wt_out[k] = c == 0 ? s : 0.0;
        if (flags) flags[k] = c;
    }
    if (k0 != 0 || !stats) return;
    u64 flagged = 0;
    int rounds = 0;
    for (int r = 0; r < niter; ++r) {
        rounds = r + 1;
        flagged += st->clipped[r];
        if (st->clipped[r] == 0u) break;
    }
    stats[0] = (double)rounds;
    stats[1] = (double)st->cls[0];
    stats[2] = (double)flagged;
    stats[3] = (double)st->cls[3];
    stats[4] = (double)st->sir;
    stats[5] = 0.0;
    stats[6] = (double)st->cls[1];
    stats[7] = (double)((u64)st->cls[0] - flagged - (u64)st->sir);
}

template <int K>
void launch_stage(gridhip_ctx *ctx, dim3 grid, const Cube &q, int round, double level, int64_t min_count, const FlagScratch &s,
                  uint8_t *c8)
{
    hipLaunchKernelGGL((st_stage_kernel<K>), grid, dim3(ST_THREADS), Stage<K>::LDS, ctx->stream, q, round, level, min_count,
                       (const u64 *)s.keys, s.codes, c8, (const FlagGroup *)s.gs, s.st);
}

size_t round256(size_t x) { return (x + 255) & ~(size_t)255; }

// the scratch of a call: flag.hip's block, the byte codes, and for the SIR operator 16 B per sample
size_t st_scratch_bytes(int64_t n, int64_t B, bool sir) { return round256(flag_scratch_bytes(n, B)) + round256((size_t)n) + (sir ? 2 * round256((size_t)n * 8) : 0); }

// q = rint(eta * 2^20)
i64 sir_q(double eta) { return (i64)__builtin_rint(eta * (double)SIR_ONE); }

int st_check(gridhip_ctx *ctx, int64_t B, int64_t T, int64_t F, int order, const double *vis, const double *model_vis,
             const double *wt_in, int64_t K, const double *levels, double eta_f, double eta_t, int64_t min_count,
             int64_t niter, const double *wt_out, const uint8_t *flags_out, const double *baseline_stats, const double *stats)
{
    bool ok = B >= 1 && T >= 1 && F >= 1 && (order == 0 || order == 1) && vis && wt_out && K >= 1 && K <= ST_MAX_STAGES && levels;
    for (int64_t k = 0; ok && k < K; ++k) ok = isfinite(levels[k]) && levels[k] > 0.0;
    ok = ok && eta_f >= 0.0 && eta_f < 1.0 && eta_t >= 0.0 && eta_t < 1.0 && min_count >= 1 && niter >= 0 && niter <= ST_MAX_ROUNDS;
    if (!ok) return fail(ctx, GRIDHIP_EINVAL, "sumthreshold: bad argument");
    // (2^18 * 2^20 * 2^20 fits an int64)
    const bool fits = B <= FLAG_MAX_GROUPS && T <= ST_MAX_ROW && F <= ST_MAX_ROW && B * T * F <= (int64_t)0xffffffffLL;
    if (fits) {  // (sizes that overflow nothing)
        const size_t n = (size_t)(B * T * F), n8 = n * 8;
        const int clash = outputs_clash({{wt_out, n8}, {flags_out, n}, {baseline_stats, (size_t)B * 32}, {stats, 64}},
                                        {{vis, 2 * n8}, {model_vis, 2 * n8}, {wt_in, n8}}, {{0, 2}});
        if (clash == 1) return fail(ctx, GRIDHIP_EINVAL, "sumthreshold: an output overlaps an input (only wt_out may be wt_in)");
        if (clash == 2) return fail(ctx, GRIDHIP_EINVAL, "sumthreshold: two outputs overlap");
    }
    if (B > FLAG_MAX_GROUPS) return fail(ctx, GRIDHIP_EUNSUPPORTED, "sumthreshold: B above %lld", (long long)FLAG_MAX_GROUPS);
    if (T > ST_MAX_ROW || F > ST_MAX_ROW) return fail(ctx, GRIDHIP_EUNSUPPORTED, "sumthreshold: T or F above 2^20");
    if (!fits) return fail(ctx, GRIDHIP_EUNSUPPORTED, "sumthreshold: B T F above 2^32 - 1");
    return GRIDHIP_OK;
}

int st_run(gridhip_ctx *ctx, const Cube &q, const double *vis, const double *model_vis, const double *wt_in, int64_t K,
           const double *levels, double eta_f, double eta_t, int64_t min_count, int64_t niter, double *wt_out,
           uint8_t *flags_out, double *baseline_stats, double *stats, void *scratch)
{
    const int64_t n = q.B * q.T * q.F;
    const FlagScratch s = flag_scratch_parts(scratch, n, q.B);
    char *rest = reinterpret_cast<char *>(scratch) + round256(flag_scratch_bytes(n, q.B));
    uint8_t *c8 = reinterpret_cast<uint8_t *>(rest);
    i64 *pn = reinterpret_cast<i64 *>(rest + round256((size_t)n)), *pmin = pn + round256((size_t)n * 8) / 8;
    // the baseline of sample k is (k / sb) % B: k / (T F) in [B][T][F], (k / F) % B in [T][B][F]
    GH_CHECK(flag_front(ctx, n, q.B, nullptr, q.sb, vis, model_vis, wt_in, 0.0, c8, s));
    const int64_t tiles = q.B * ((q.T + ST_TILE_T - 1) / ST_TILE_T) * ((q.F + ST_TILE_F - 1) / ST_TILE_F);
    const int64_t most = (int64_t)ctx->num_cu * 8;
    const dim3 tgrid((unsigned)(tiles < most ? tiles : most));
    if (niter == 0) GH_CHECK(flag_select(ctx, n, q.B, -1, levels[0], true, min_count, baseline_stats, s));
    for (int r = 0; r < (int)niter; ++r) {
        GH_CHECK(flag_select(ctx, n, q.B, r, levels[0], true, min_count, baseline_stats, s));
        for (int k = 0; k < (int)K; ++k) switch (k) {
                case 0: launch_stage<0>(ctx, tgrid, q, r, levels[k], min_count, s, c8); break;
                case 1: launch_stage<1>(ctx, tgrid, q, r, levels[k], min_count, s, c8); break;
                case 2: launch_stage<2>(ctx, tgrid, q, r, levels[k], min_count, s, c8); break;
                case 3: launch_stage<3>(ctx, tgrid, q, r, levels[k], min_count, s, c8); break;
                case 4: launch_stage<4>(ctx, tgrid, q, r, levels[k], min_count, s, c8); break;
                case 5: launch_stage<5>(ctx, tgrid, q, r, levels[k], min_count, s, c8); break;
                default: launch_stage<6>(ctx, tgrid, q, r, levels[k], min_count, s, c8); break;
            }
    }
    for (int dir = 0; dir < 2; ++dir) {
        const i64 qq = sir_q(dir ? eta_t : eta_f);
        if ((dir ? eta_t : eta_f) == 0.0) continue;
        const int64_t rows = dir ? q.B * q.F : q.B * q.T;
        const dim3 rgrid = grid_for(ctx, rows * 64);
        hipLaunchKernelGGL(st_sir_fwd_kernel, rgrid, dim3(ST_THREADS), 0, ctx->stream, q, dir, qq, (const uint8_t *)c8, pn, pmin);
        hipLaunchKernelGGL(st_sir_bwd_kernel, rgrid, dim3(ST_THREADS), 0, ctx->stream, q, dir, c8, (const i64 *)pn,
                           (const i64 *)pmin, s.st);
    }
    hipLaunchKernelGGL(st_final_kernel, grid_for(ctx, n), dim3(256), 0, ctx->stream, n, (int)niter, (const uint8_t *)c8, wt_in,
                       wt_out, flags_out, (const FlagState *)s.st, stats);
    GH_CHECK_HIP(ctx, hipGetLastError());
    return GRIDHIP_OK;
}

int st_any(gridhip_ctx *ctx, bool dev, int64_t B, int64_t T, int64_t F, int order, const double *vis, const double *model_vis,
           const double *wt_in, int64_t K, const double *levels, double eta_f, double eta_t, int64_t min_count, int64_t niter,
           double *wt_out, uint8_t *flags_out, double *baseline_stats, double *stats)
{
    if (!ctx) return GRIDHIP_EINVAL;
    GH_CHECK(st_check(ctx, B, T, F, order, vis, model_vis, wt_in, K, levels, eta_f, eta_t, min_count, niter, wt_out, flags_out,
                      baseline_stats, stats));
    GH_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    Cube q;
    q.B = B, q.T = T, q.F = F;
    q.sb = order == 0 ? T * F : F;
    q.st = order == 0 ? F : B * F;
    const int64_t n = B * T * F;
    const size_t n8 = (size_t)n * 8;
    DevBuf scratch;
    GH_CHECK(scratch.alloc(ctx, st_scratch_bytes(n, B, eta_f > 0.0 || eta_t > 0.0)));
    Staged sg(ctx, dev);
    vis = sg.in(vis, 2 * n8), model_vis = sg.in(model_vis, 2 * n8), wt_in = sg.in(wt_in, n8);
    wt_out = sg.out(wt_out, n8), flags_out = sg.out(flags_out, (size_t)n), baseline_stats = sg.out(baseline_stats, (size_t)B * 32);
    stats = sg.out(stats, 64);
    GH_CHECK(sg.status());
    GH_CHECK(st_run(ctx, q, vis, model_vis, wt_in, K, levels, eta_f, eta_t, min_count, niter, wt_out, flags_out, baseline_stats,
                    stats, scratch.p));
    return sg.finish();
}

}  // namespace

}  // namespace gridhip

using namespace gridhip;

extern "C" {

int gridhip_sumthreshold(gridhip_ctx *ctx, int64_t B, int64_t T, int64_t F, int order, const double *vis,
                         const double *model_vis, const double *wt_in, int64_t K, const double *levels, double eta_f,
                         double eta_t, int64_t min_count, int64_t niter, double *wt_out, uint8_t *flags_out,
                         double *baseline_stats, double *stats)
{
    return st_any(ctx, false, B, T, F, order, vis, model_vis, wt_in, K, levels, eta_f, eta_t, min_count, niter, wt_out,
                  flags_out, baseline_stats, stats);
}

int gridhip_sumthreshold_dev(gridhip_ctx *ctx, int64_t B, int64_t T, int64_t F, int order, const double *vis,
                             const double *model_vis, const double *wt_in, int64_t K, const double *levels, double eta_f,
                             double eta_t, int64_t min_count, int64_t niter, double *wt_out, uint8_t *flags_out,
                             double *baseline_stats, double *stats)
{
    return st_any(ctx, true, B, T, F, order, vis, model_vis, wt_in, K, levels, eta_f, eta_t, min_count, niter, wt_out,
                  flags_out, baseline_stats, stats);
}

int gridhip_sumthreshold_tile(int64_t *tile_t, int64_t *tile_f)
{
    if (!tile_t || !tile_f) return GRIDHIP_EINVAL;
    *tile_t = ST_TILE_T, *tile_f = ST_TILE_F;
    return GRIDHIP_OK;
}

}  // extern "C"
