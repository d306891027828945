// Residual flagging (include/gridhip.h, "residual flagging"): per group of a visibility stream, the lower median and the
// median absolute deviation of the residual amplitudes, exact and read-back free, and the weights of a stream whose
// outliers are clipped - the one step of a major-cycle loop that decides that a sample is bad.
//
// Both statistics are order statistics of 64-bit keys (a >= +0.0 and d = |a - med| >= +0.0, so a double's own bits order
// them), found for ALL groups at once by a segmented most-significant-digit radix select with 8-bit digits (noise.hip is
// the same select over one image).  One call is
//     flag_init_kernel                    zeroes the [G][256] bin table and the state block (a kernel: no memset node)
//     flag_front_kernel                   one pass over vis, model, wt, group (40 B): the classes 1 to 4, and per
//                                         visibility the 8-byte key of a and a 4-byte group code (FLAG_DEAD: takes part in
//                                         nothing, its weight becomes +0.0; FLAG_LEFT: left alone, its weight stays)
//     niter x { 8 x { flag_hist_kernel<LDS, false>   streams key and code (12 B): one digit of a over the participants
//                                                    whose higher digits equal their group's prefix
//                     flag_pick_kernel               one wave per group: the digit that holds the group's rank goes
//                                                    into its prefix, the rank is lowered, the bins walked are zeroed }
//               8 x { flag_hist_kernel<LDS, true>, flag_pick_kernel }   the same over d, the median read from the state
//               flag_clip_kernel                     a > T_g: code 16 + r, the participant retires (FLAG_DEAD) }
//     flag_final_kernel                   wt_out from wt_in and the codes; the 8 stats
// 2 + 33 niter + 1 launches whatever the data hold (niter = 0: one histogram and one pick for the groups' counts).
// The histogram has two paths, chosen by G alone.  G <= FLAG_LDS_GROUPS: a work-group keeps G x 256 32-bit bins in
// dynamic LDS (1 KB per group, so a small G zeroes and walks a small table) and adds its non-zero bins to the global table.
// Above: every lane adds to the global [G][256] table directly - the adds are spread over G x 256 addresses.
// Integer atomics only.  A group's prefix, rank, count, median, MAD and threshold sit in a 40-byte row of a state table.
// The stop test lives on the device (clean.hip's scheme): round r counts what it clips in its own counter, every launch
// of round r + 1 reads that counter first and returns when it is zero - the zero counter IS the stop flag, and a round
// that never ran leaves its counter zero for the rounds after it.
// The front pass (flag_front) and the select of a round (flag_select) also serve time-frequency flagging (sumthreshold.hip),
// through imaging.h: its groups are the baselines of a dense cube, found from the sample's index, and its threshold is
// nsigma * sigma_g without the median.
// Determinism: counts, key comparisons and one rounded expression per output (contraction off); no floating-point atomic
// and no sum of doubles anywhere in this file.  The result is the same bits on every run and the bits a host sort gives.
#include "common.h"
#include "imaging.h"

namespace gridhip {

namespace {

typedef unsigned long long u64;
typedef unsigned int u32;

constexpr u64 EXP_MASK = 0x7ff0000000000000ULL;
static_assert(FLAG_MAX_GROUPS < (int64_t)FLAG_LEFT, "a group code holds every group and the two reserved values");

struct FlagLayout {
    size_t state, groups, bins, keys, codes, total;
};

size_t round256(size_t x) { return (x + 255) & ~(size_t)255; }

// keys and codes are padded by two or three dead slots to an even count: the streaming passes read them two at a time
FlagLayout layout(int64_t n, int64_t G)
{
    FlagLayout l;
    const size_t slots = ((size_t)n + 3) & ~(size_t)1;
    l.state = 0;
    l.groups = sizeof(FlagState);
    l.bins = l.groups + round256((size_t)G * sizeof(FlagGroup));
    l.keys = l.bins + (size_t)G * 256 * sizeof(u32);
    l.codes = l.keys + round256(slots * 8);
    l.total = l.codes + round256(slots * 4);
    return l;
}

// words: the 32-bit words of the bin table (a multiple of 4).  The two slots behind the n codes are dead (layout).
__global__ void __launch_bounds__(256)
    flag_init_kernel(int64_t words, int64_t n, FlagState *st, u32 *__restrict__ bins, u64 *__restrict__ keys,
                     u32 *__restrict__ codes)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, step = (int64_t)gridDim.x * blockDim.x;
    uint4 *b4 = reinterpret_cast<uint4 *>(bins);
    for (int64_t i = t; i < words / 4; i += step) b4[i] = make_uint4(0u, 0u, 0u, 0u);
    if (t < (int64_t)(sizeof(FlagState) / 4)) reinterpret_cast<u32 *>(st)[t] = 0u;
    if (t < 2) keys[n + t] = 0ull, codes[n + t] = FLAG_DEAD;
}

// The classes 1 to 4 (the first that applies), the key and the group code of every visibility; flags may be null.
// cube_div > 0: the group is (k / cube_div) % G, the baseline of a dense cube (imaging.h), and `group` is not read.
__global__ void __launch_bounds__(256)
    flag_front_kernel(int64_t n, int64_t G, const int64_t *__restrict__ group, int64_t cube_div, const double2 *__restrict__ vis,
                      const double2 *__restrict__ mod, const double *__restrict__ wt, double amax, u64 *__restrict__ keys,
                      u32 *__restrict__ codes, uint8_t *__restrict__ flags, FlagState *st)
{
#pragma clang fp contract(off)
    const int64_t k0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, step = (int64_t)gridDim.x * blockDim.x;
    u32 c[5] = {0u, 0u, 0u, 0u, 0u};
    for (int64_t k = k0; k < n; k += step) {
        const double s = wt ? wt[k] : 1.0;
        const int64_t g = cube_div > 0 ? (int64_t)(((u64)k / (u64)cube_div) % (u64)G) : group ? group[k] : 0;
        int cl = 0;
        u64 key = 0ull;
        if (!(s > 0.0)) {
            cl = 1;
        } else if (g < 0 || g >= G) {
            cl = 2;
        } else {
            double2 r = vis[k];
            if (mod) {
                const double2 m = mod[k];
                r = make_double2(r.x - m.x, r.y - m.y);
            }
            const double a = sqrt(r.x * r.x + r.y * r.y);
            key = __builtin_bit_cast(u64, a);
            if ((key & EXP_MASK) == EXP_MASK)
                cl = 3;
            else if (amax > 0.0 && a > amax)
                cl = 4;
        }
        keys[k] = key;
        codes[k] = cl == 0 ? (u32)g : cl == 2 ? FLAG_LEFT : FLAG_DEAD;
        if (flags) flags[k] = (uint8_t)cl;
#pragma unroll
        for (int j = 0; j < 5; ++j) c[j] += (u32)(cl == j);
    }
    for (int j = 0; j < 5; ++j) flag_wave_count(c[j], &st->cls[j]);
}

// One digit (the 8 bits from `shift` up) of the key of every participant whose bits above the digit equal its group's
// prefix.  MAD: the key is that of |a - med_g|.  A thread takes the slots 2 j, 2 j + 1 for j = t, t + T, ... (a 16-byte
// and an 8-byte load).  LDS: dynamic LDS of G x 256 32-bit bins, flushed to the global table where not zero.
template <bool LDS, bool MAD>
__global__ void __launch_bounds__(256)
    flag_hist_kernel(int64_t pairs, int G, int shift, int round, const u64 *__restrict__ keys, const u32 *__restrict__ codes,
                     const FlagGroup *__restrict__ gs, const FlagState *st, u32 *__restrict__ bins)
{
#pragma clang fp contract(off)
    extern __shared__ u32 lbins[];
    if (flag_stopped(st, round)) return;
    const int hi = shift + 8, nb = G * 256;
    if (LDS) {
        for (int i = threadIdx.x; i < nb; i += 256) lbins[i] = 0u;
        __syncthreads();
    }
    const ulonglong2 *k2 = reinterpret_cast<const ulonglong2 *>(keys);
    const uint2 *c2 = reinterpret_cast<const uint2 *>(codes);
    const int64_t T = (int64_t)gridDim.x * 256;
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < pairs; j += T) {
        const ulonglong2 kk = k2[j];
        const uint2 cc = c2[j];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const u32 g = e ? cc.y : cc.x;
            if (g >= FLAG_LEFT) continue;
            u64 key = e ? kk.y : kk.x;
            if (MAD) key = __builtin_bit_cast(u64, fabs(__builtin_bit_cast(double, key) - gs[g].med));
            if (hi < 64 && ((key ^ gs[g].prefix) >> hi) != 0) continue;
            const u32 bin = g * 256u + ((u32)(key >> shift) & 255u);
            if (LDS)
                atomicAdd(&lbins[bin], 1u);
            else
                atomicAdd(&bins[bin], 1u);
        }
    }
    if (LDS) {
        __syncthreads();
        for (int i = threadIdx.x; i < nb; i += 256) {
            const u32 c = lbins[i];
            if (c) atomicAdd(&bins[i], c);
        }
    }
}

// One wave per group, four groups per work-group.  Lane l owns the bins 4 l .. 4 l + 3 of its group (one 16-byte load):
// an inclusive scan of the lanes' sums by shuffles tells the one lane whose bins hold the wanted rank, which walks them,
// puts the digit into the prefix and lowers the rank.  Every lane zeroes the bins it found not zero.
// first: the first pass of a round - n_g is the sum of all bins and the wanted rank (n_g - 1) / 2; a group that is empty
// gets { 0, NaN, NaN, +Inf } and is skipped by every later pick of the round (nothing is ever added to its bins).
// last: 1 - the prefix is the median: into the state, and the second selection starts from an empty prefix and the same
// rank; 2 - the prefix is the MAD: T_g (sigma_only: nsigma * sigma_g without the median, sumthreshold.hip's chi_0) and
// the group's stats row; 3 (niter = 0, with first) - the count alone.
__global__ void __launch_bounds__(256)
    flag_pick_kernel(int64_t G, int shift, int first, int last, int round, double nsigma, int sigma_only, int64_t min_count, FlagGroup *gs,
                     u32 *bins, const FlagState *st, double *__restrict__ group_stats)
{
#pragma clang fp contract(off)
    if (flag_stopped(st, round)) return;
    const int64_t g = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= G) return;
    const int lane = threadIdx.x & 63;
    FlagGroup *s = gs + g;
    // (the state is read by every lane here and written by one lane below: the wave runs these in program order)
    const u32 n0 = first ? 0u : s->n, rank0 = first ? 0u : s->rank;
    const u64 prefix0 = first ? 0ull : s->prefix;
    if (!first && n0 == 0u) return;
    uint4 *row = reinterpret_cast<uint4 *>(bins + g * 256) + lane;
    const uint4 b = *row;
    const u32 sum = b.x + b.y + b.z + b.w;
    if (sum) *row = make_uint4(0u, 0u, 0u, 0u);
    u32 inc = sum;
    for (int off = 1; off < 64; off <<= 1) {
        const u32 o = __shfl_up(inc, off);
        if (lane >= off) inc += o;
    }
    const u32 total = __shfl(inc, 63), exc = inc - sum;
    const double nan = __builtin_nan(""), inf = __builtin_inf();
    if (first && (total == 0u || last == 3)) {
        if (lane == 0) {
            s->n = total, s->rank = 0u, s->prefix = 0ull;
            s->med = nan, s->mad = nan, s->T = inf;
            if (group_stats) {
                double *o = group_stats + 4 * g;
                o[0] = (double)total, o[1] = nan, o[2] = nan, o[3] = inf;
            }
        }
        return;
    }
    const u32 n = first ? total : n0, rank = first ? (total - 1u) / 2u : rank0;
    if (!(sum > 0u && rank >= exc && rank < exc + sum)) return;  // (exactly one lane goes on)
    const u32 mine[4] = {b.x, b.y, b.z, b.w};
    u32 below = exc;
    int d = -1;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (d < 0 && rank < below + mine[j]) d = 4 * lane + j;
        if (d < 0) below += mine[j];
    }
    const u64 prefix = prefix0 | ((u64)d << shift);
    if (first) s->n = n;
    if (last == 0) {
        s->prefix = prefix;
        s->rank = rank - below;
    } else if (last == 1) {
        s->med = __builtin_bit_cast(double, prefix);
        s->prefix = 0ull;
        s->rank = (n - 1u) / 2u;
    } else {
        const double med = s->med, mad = __builtin_bit_cast(double, prefix);
        const double sigma = 1.4826 * mad;
        const double ns = nsigma * sigma;
        const double T = ((int64_t)n < min_count || sigma == 0.0) ? inf : sigma_only ? ns : med + ns;
        s->mad = mad;
        s->T = T;
        if (group_stats) {
            double *o = group_stats + 4 * g;
            o[0] = (double)n, o[1] = med, o[2] = mad, o[3] = T;
        }
    }
}

// Round `round`: a participant with a > T_g gets the code 16 + round and retires.  What the round clips is counted in
// its own counter, which the launches of the next round read first.
__global__ void __launch_bounds__(256)
    flag_clip_kernel(int64_t pairs, int round, const u64 *__restrict__ keys, u32 *codes, const FlagGroup *__restrict__ gs,
                     FlagState *st, uint8_t *__restrict__ flags)
{
    if (flag_stopped(st, round)) return;
    const ulonglong2 *k2 = reinterpret_cast<const ulonglong2 *>(keys);
    const uint2 *c2 = reinterpret_cast<const uint2 *>(codes);  // (a slot is read and then written by the same lane)
    const int64_t T = (int64_t)gridDim.x * 256;
    u32 count = 0u;
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < pairs; j += T) {
        const ulonglong2 kk = k2[j];
        const uint2 cc = c2[j];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const u32 g = e ? cc.y : cc.x;
            if (g >= FLAG_LEFT) continue;
            if (!(__builtin_bit_cast(double, e ? kk.y : kk.x) > gs[g].T)) continue;
            codes[2 * j + e] = FLAG_DEAD;
            if (flags) flags[2 * j + e] = (uint8_t)(16 + round);
            count += 1u;
        }
    }
    flag_wave_count(count, &st->clipped[round]);
}

// wt_out = the data weight (1 without data weights) where the visibility is kept or left alone, else +0.0.  wt_out may be
// wt_in itself (element k is read before it is written, by the same lane): no __restrict__ on those.  The first thread
// writes the 8 stats when they are asked for.
__global__ void __launch_bounds__(256)
    flag_final_kernel(int64_t n, int niter, const u32 *__restrict__ codes, const double *wt_in, double *wt_out,
                      const FlagState *st, double *__restrict__ stats)
{
    const int64_t k0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, step = (int64_t)gridDim.x * blockDim.x;
    for (int64_t k = k0; k < n; k += step) {
        const double s = wt_in ? wt_in[k] : 1.0;
        wt_out[k] = codes[k] == FLAG_DEAD ? 0.0 : s;
    }
    if (k0 != 0 || !stats) return;
    u64 clipped = 0;
    int rounds = 0;
    for (int r = 0; r < niter; ++r) {
        rounds = r + 1;
        clipped += st->clipped[r];
        if (st->clipped[r] == 0u) break;
    }
    stats[0] = (double)rounds;
    stats[1] = (double)st->cls[0];
    stats[2] = (double)clipped;
    stats[3] = (double)st->cls[3];
    stats[4] = (double)st->cls[4];
    stats[5] = (double)st->cls[2];
    stats[6] = (double)st->cls[1];
    stats[7] = (double)((u64)st->cls[0] - clipped);
}

template <bool LDS>
void launch_hist(gridhip_ctx *ctx, dim3 grid, size_t lds, bool mad, int64_t pairs, int G, int shift, int round,
                 const u64 *keys, const u32 *codes, const FlagGroup *gs, const FlagState *st, u32 *bins)
{
    if (mad)
        hipLaunchKernelGGL((flag_hist_kernel<LDS, true>), grid, dim3(256), lds, ctx->stream, pairs, G, shift, round, keys, codes,
                           gs, st, bins);
    else
        hipLaunchKernelGGL((flag_hist_kernel<LDS, false>), grid, dim3(256), lds, ctx->stream, pairs, G, shift, round, keys,
                           codes, gs, st, bins);
}

}  // namespace

int flag_check(gridhip_ctx *ctx, int64_t n, int64_t G, const int64_t *group, const double *vis, const double *model_vis,
               const double *wt_in, double nsigma, double amax, int64_t min_count, int64_t niter, const double *wt_out,
               const uint8_t *flags_out, const double *group_stats, const double *stats)
{
    if (n < 0 || G < 1 || (!group && G != 1) || (n > 0 && (!vis || !wt_out)) || !(nsigma > 0.0) || !isfinite(nsigma) ||
        !(amax >= 0.0) || min_count < 1 || niter < 0 || niter > FLAG_MAX_ROUNDS)
        return fail(ctx, GRIDHIP_EINVAL, "flag_residuals: bad argument");
    if (G <= FLAG_MAX_GROUPS && n <= (int64_t)0xffffffffLL) {  // (sizes that overflow nothing)
        const size_t n8 = (size_t)n * 8;
        const int clash = outputs_clash({{wt_out, n8}, {flags_out, (size_t)n}, {group_stats, (size_t)G * 32}, {stats, 64}},
                                        {{group, n8}, {vis, 2 * n8}, {model_vis, 2 * n8}, {wt_in, n8}}, {{0, 3}});
        if (clash == 1)
            return fail(ctx, GRIDHIP_EINVAL, "flag_residuals: an output overlaps an input (only wt_out may be wt_in)");
        if (clash == 2) return fail(ctx, GRIDHIP_EINVAL, "flag_residuals: two outputs overlap");
    }
    if (G > FLAG_MAX_GROUPS) return fail(ctx, GRIDHIP_EUNSUPPORTED, "flag_residuals: G above %lld", (long long)FLAG_MAX_GROUPS);
    if (n > (int64_t)0xffffffffLL) return fail(ctx, GRIDHIP_EUNSUPPORTED, "flag_residuals: n above 2^32 - 1");
    return GRIDHIP_OK;
}

size_t flag_scratch_bytes(int64_t n, int64_t G) { return layout(n, G).total; }

FlagScratch flag_scratch_parts(void *scratch, int64_t n, int64_t G)
{
    const FlagLayout l = layout(n, G);
    char *base = reinterpret_cast<char *>(scratch);
    FlagScratch s;
    s.st = reinterpret_cast<FlagState *>(base + l.state);
    s.gs = reinterpret_cast<FlagGroup *>(base + l.groups);
    s.bins = reinterpret_cast<u32 *>(base + l.bins);
    s.keys = reinterpret_cast<u64 *>(base + l.keys);
    s.codes = reinterpret_cast<u32 *>(base + l.codes);
    return s;
}

int flag_front(gridhip_ctx *ctx, int64_t n, int64_t G, const int64_t *group, int64_t cube_div, const double *vis,
               const double *model_vis, const double *wt_in, double amax, uint8_t *flags_out, const FlagScratch &s)
{
    const int64_t words = G * 256;
    hipLaunchKernelGGL(flag_init_kernel, grid_for(ctx, words / 4), dim3(256), 0, ctx->stream, words, n, s.st, s.bins, s.keys,
                       s.codes);
    hipLaunchKernelGGL(flag_front_kernel, grid_for(ctx, n), dim3(256), 0, ctx->stream, n, G, group, cube_div,
                       (const double2 *)vis, (const double2 *)model_vis, wt_in, amax, s.keys, s.codes, flags_out, s.st);
    GH_CHECK_HIP(ctx, hipGetLastError());
    return GRIDHIP_OK;
}

int flag_select(gridhip_ctx *ctx, int64_t n, int64_t G, int round, double level, bool sigma_only, int64_t min_count,
                double *group_stats, const FlagScratch &s)
{
    const bool lds = G <= FLAG_LDS_GROUPS;
    const size_t lds_bytes = lds ? (size_t)G * 1024 : 0;
    if (!ctx->img->flag_lds_raised) {  // (64 KB of dynamic LDS at G = 64: the functions are told so once)
        GH_CHECK_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(flag_hist_kernel<true, false>),
                                              hipFuncAttributeMaxDynamicSharedMemorySize, FLAG_LDS_GROUPS * 1024));
        GH_CHECK_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(flag_hist_kernel<true, true>),
                                              hipFuncAttributeMaxDynamicSharedMemorySize, FLAG_LDS_GROUPS * 1024));
        ctx->img->flag_lds_raised = true;
    }
    const int64_t pairs = (n + 1) / 2;
    const dim3 pgrid = grid_for(ctx, pairs), kgrid((unsigned)((G + 3) / 4));
    // the LDS path zeroes and walks its table in every work-group: fewer, longer-lived work-groups the larger the table
    int64_t hwg = (pairs + 1023) / 1024, most = (int64_t)ctx->num_cu * (lds_bytes <= 16384 ? 4 : 2);
    if (hwg < 1) hwg = 1;
    if (hwg > most) hwg = most;
    const dim3 hgrid = lds ? dim3((unsigned)hwg) : pgrid;
    const auto hist = [&](bool mad, int shift, int r) {
        if (lds)
            launch_hist<true>(ctx, hgrid, lds_bytes, mad, pairs, (int)G, shift, r, s.keys, s.codes, s.gs, s.st, s.bins);
        else
            launch_hist<false>(ctx, hgrid, 0, mad, pairs, (int)G, shift, r, s.keys, s.codes, s.gs, s.st, s.bins);
    };
    const int so = sigma_only ? 1 : 0;
    if (round < 0) {  // the groups' counts alone
        hist(false, 56, 0);
        hipLaunchKernelGGL(flag_pick_kernel, kgrid, dim3(256), 0, ctx->stream, G, 56, 1, 3, 0, level, so, min_count, s.gs,
                           s.bins, (const FlagState *)s.st, group_stats);
    } else {
        for (int sel = 0; sel < 2; ++sel)
            for (int p = 0; p < 8; ++p) {
                const int shift = 56 - 8 * p;
                hist(sel == 1, shift, round);
                hipLaunchKernelGGL(flag_pick_kernel, kgrid, dim3(256), 0, ctx->stream, G, shift, (int)(sel == 0 && p == 0),
                                   p == 7 ? sel + 1 : 0, round, level, so, min_count, s.gs, s.bins, (const FlagState *)s.st,
                                   group_stats);
            }
    }
    GH_CHECK_HIP(ctx, hipGetLastError());
    return GRIDHIP_OK;
}

int flag_run(gridhip_ctx *ctx, int64_t n, int64_t G, const int64_t *group, const double *vis, const double *model_vis,
             const double *wt_in, double nsigma, double amax, int64_t min_count, int64_t niter, double *wt_out,
             uint8_t *flags_out, double *group_stats, double *stats, void *scratch)
{
    const FlagScratch s = flag_scratch_parts(scratch, n, G);
    const int64_t pairs = (n + 1) / 2;
    GH_CHECK(flag_front(ctx, n, G, group, 0, vis, model_vis, wt_in, amax, flags_out, s));
    if (niter == 0) GH_CHECK(flag_select(ctx, n, G, -1, nsigma, false, min_count, group_stats, s));
    for (int r = 0; r < (int)niter; ++r) {
        GH_CHECK(flag_select(ctx, n, G, r, nsigma, false, min_count, group_stats, s));
        hipLaunchKernelGGL(flag_clip_kernel, grid_for(ctx, pairs), dim3(256), 0, ctx->stream, pairs, r, (const u64 *)s.keys,
                           s.codes, (const FlagGroup *)s.gs, s.st, flags_out);
    }
    hipLaunchKernelGGL(flag_final_kernel, grid_for(ctx, n), dim3(256), 0, ctx->stream, n, (int)niter, (const u32 *)s.codes,
                       wt_in, wt_out, (const FlagState *)s.st, stats);
    GH_CHECK_HIP(ctx, hipGetLastError());
    return GRIDHIP_OK;
}

}  // namespace gridhip

using namespace gridhip;

namespace {

int flag_any(gridhip_ctx *ctx, bool dev, int64_t n, int64_t G, const int64_t *group, const double *vis,
             const double *model_vis, const double *wt_in, double nsigma, double amax, int64_t min_count, int64_t niter,
             double *wt_out, uint8_t *flags_out, double *group_stats, double *stats)
{
    if (!ctx) return GRIDHIP_EINVAL;
    GH_CHECK(flag_check(ctx, n, G, group, vis, model_vis, wt_in, nsigma, amax, min_count, niter, wt_out, flags_out,
                        group_stats, stats));
    GH_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n8 = (size_t)n * 8;
    DevBuf scratch;
    GH_CHECK(scratch.alloc(ctx, flag_scratch_bytes(n, G)));
    Staged st(ctx, dev);
    group = st.in(group, n8), vis = st.in(vis, 2 * n8), model_vis = st.in(model_vis, 2 * n8), wt_in = st.in(wt_in, n8);
    wt_out = st.out(wt_out, n8), flags_out = st.out(flags_out, (size_t)n), group_stats = st.out(group_stats, (size_t)G * 32);
    stats = st.out(stats, 64);
    GH_CHECK(st.status());
    GH_CHECK(flag_run(ctx, n, G, group, vis, model_vis, wt_in, nsigma, amax, min_count, niter, wt_out, flags_out, group_stats,
                      stats, scratch.p));
    return st.finish();
}

}  // namespace

extern "C" {

int gridhip_flag_residuals_dev(gridhip_ctx *ctx, int64_t n, int64_t G, const int64_t *group, const double *vis,
                               const double *model_vis, const double *wt_in, double nsigma, double amax, int64_t min_count,
                               int64_t niter, double *wt_out, uint8_t *flags_out, double *group_stats, double *stats)
{
    return flag_any(ctx, true, n, G, group, vis, model_vis, wt_in, nsigma, amax, min_count, niter, wt_out, flags_out,
                    group_stats, stats);
}

int gridhip_flag_residuals(gridhip_ctx *ctx, int64_t n, int64_t G, const int64_t *group, const double *vis,
                           const double *model_vis, const double *wt_in, double nsigma, double amax, int64_t min_count,
                           int64_t niter, double *wt_out, uint8_t *flags_out, double *group_stats, double *stats)
{
    return flag_any(ctx, false, n, G, group, vis, model_vis, wt_in, nsigma, amax, min_count, niter, wt_out, flags_out,
                    group_stats, stats);
}

}  // extern "C"
