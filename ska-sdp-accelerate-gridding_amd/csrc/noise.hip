// Robust image statistics (include/gridhip.h, "image statistics"): the lower median and the median absolute deviation of
// an N x N image, exact and read-back free, so that a minor cycle can stop at n sigma of the map it cleans.
//
// Both are order statistics of 64-bit keys (ordered_bits: a double's bits, all flipped for a negative value, the sign bit
// flipped otherwise), found by a most-significant-digit radix select, never a sort.  One call is
//     noise_init_kernel                      zeroes the bin table and the state block
//     P x { noise_hist_kernel<0 | 1>         one pass over the image: the histogram of one digit of the key over the cells
//                                            whose higher digits equal the prefix chosen so far
//           noise_scan_kernel                one work-group: scans the bins, takes the digit that holds the wanted rank into
//                                            the prefix, lowers the rank by the cells below it, zeroes the bins again }
//     P x { noise_hist_kernel<2>, noise_scan_kernel }    the same over d = |x - median|, the median read from the state
// with P = ceil(64 / digit bits) passes per selection: 1 + 4 P launches whatever the image holds.  The first pass also
// takes n (the sum of its bins), the smallest and largest key and the number of non-finite cells skipped; the last scan
// writes the 8 stats.
// A work-group histograms into LDS with 32-bit integer atomics and then adds its non-zero bins to the 64-bit table in
// global memory with integer atomics; the smallest and largest key are reduced with shuffles and LDS, one row per
// work-group, and the scan kernel reduces the rows (group_best's shape).  Integer counts and key comparisons do not depend
// on the schedule and there is no floating-point atomic, no sum of doubles and no comparison of doubles in this file: the
// result is the same bits on every run, and the bits a sort of the keys on the host gives.
// The digit is 13 bits wide (32 KB of LDS bins, 5 + 5 passes) unless the context option "noise_bits" says 8 (1 KB, 8 + 8
// passes); DESIGN.md section 9 has the measurement behind the default.
#include "common.h"
#include "imaging.h"

namespace gridhip {

namespace {

typedef unsigned long long u64;

constexpr int NOISE_MAX_BITS = 13;
constexpr u64 EXP_MASK = 0x7ff0000000000000ULL;

struct NoiseState {  // 64 bytes at the head of the scratch block
    u64 prefix;   // the digits of the wanted key chosen so far (the lower bits zero)
    u64 rank;     // the wanted rank among the cells whose higher digits equal the prefix
    u64 n;        // the cells that take part
    u64 skipped;  // non-finite cells inside border and mask
    u64 kmin, kmax;  // the smallest and the largest key
    double median;
    u64 pad;
};

struct NoiseLayout {
    size_t state, bins, rows, total;
    int nwg;
};

// the scratch is laid out for the widest digit and the largest grid, whatever the option says: a change of the option
// allocates nothing
NoiseLayout layout(gridhip_ctx *ctx)
{
    NoiseLayout l;
    l.nwg = ctx->num_cu * 4;
    l.state = 256;
    l.bins = ((size_t)8 << NOISE_MAX_BITS);
    l.rows = (size_t)l.nwg * 3 * sizeof(u64);
    l.total = l.state + l.bins + l.rows;
    return l;
}

__global__ void __launch_bounds__(256) noise_init_kernel(NoiseState *st, u64 *bins, int nbins)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    for (int i = t; i < nbins; i += gridDim.x * blockDim.x) bins[i] = 0;
    if (t < (int)(sizeof(NoiseState) / 8)) reinterpret_cast<u64 *>(st)[t] = 0;
}

// MODE 0: the first pass of the first selection - every cell that takes part is counted, and the work-group's smallest
// and largest key and its count of skipped cells go to its row.  MODE 1: a later pass of the first selection.  MODE 2: a
// pass of the second selection, the key that of |x - median|.
// A cell is counted when the bits of its key above the digit (`hi` and up) equal the prefix's.  A thread walks the flat
// indices t, t + T, t + 2 T ... (T the threads of the grid) and keeps (y, x) beside the index without a division per cell.
// dynamic LDS: (1 << width) 32-bit bins
template <int MODE>
__global__ void __launch_bounds__(256)
    noise_hist_kernel(int64_t N, int64_t border, const double *__restrict__ image, const uint8_t *__restrict__ mask,
                      int shift, int width, const NoiseState *st, u64 *__restrict__ bins, u64 *__restrict__ rows)
{
#pragma clang fp contract(off)
    extern __shared__ unsigned int lbins[];
    __shared__ u64 sh[3][4];
    if (MODE != 0 && st->n == 0) return;
    const int nb = 1 << width, hi = shift + width;
    const u64 prefix = MODE == 0 ? 0 : st->prefix;
    const double median = MODE == 2 ? st->median : 0.0;
    for (int i = threadIdx.x; i < nb; i += 256) lbins[i] = 0;
    __syncthreads();
    const int64_t cells = N * N, T = (int64_t)gridDim.x * 256;
    const int64_t sy = T / N, sx = T % N;
    int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int64_t y = k / N, x = k % N;
    u64 kmin = ~(u64)0, kmax = 0, skipped = 0;
    for (; k < cells; k += T) {
        if (y >= border && y < N - border && x >= border && x < N - border && (!mask || mask[k] != 0)) {
            const double v = image[k];
            const u64 b = __builtin_bit_cast(u64, v);
            if ((b & EXP_MASK) != EXP_MASK) {
                const u64 key = MODE == 2 ? ordered_bits(fabs(v - median)) : ordered_bits(v);
                if (MODE == 0) {
                    kmin = key < kmin ? key : kmin;
                    kmax = key > kmax ? key : kmax;
                }
                if (hi >= 64 || ((key ^ prefix) >> hi) == 0) atomicAdd(&lbins[(unsigned)(key >> shift) & (unsigned)(nb - 1)], 1u);
            } else if (MODE == 0) {
                skipped += 1;
            }
        }
        y += sy, x += sx;
        if (x >= N) x -= N, y += 1;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nb; i += 256) {
        const unsigned int c = lbins[i];
        if (c) atomicAdd(&bins[i], (u64)c);
    }
    if (MODE == 0) {
        for (int off = 32; off > 0; off >>= 1) {
            const u64 a = __shfl_down(kmin, off), b = __shfl_down(kmax, off);
            kmin = a < kmin ? a : kmin;
            kmax = b > kmax ? b : kmax;
            skipped += __shfl_down(skipped, off);
        }
        const int wave = threadIdx.x >> 6;
        if ((threadIdx.x & 63) == 0) sh[0][wave] = kmin, sh[1][wave] = kmax, sh[2][wave] = skipped;
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int w = 1; w < 4; ++w) {
                kmin = sh[0][w] < kmin ? sh[0][w] : kmin;
                kmax = sh[1][w] > kmax ? sh[1][w] : kmax;
                skipped += sh[2][w];
            }
            rows[3 * blockIdx.x + 0] = kmin;
            rows[3 * blockIdx.x + 1] = kmax;
            rows[3 * blockIdx.x + 2] = skipped;
        }
    }
}

// One work-group of 1024 threads.  Thread t owns the bins [t * per, (t + 1) * per); an exclusive scan of the threads'
// sums (shuffles inside a wave, the waves' totals through LDS) tells the one thread whose bins hold the wanted rank, which
// walks them, puts the digit into the prefix and lowers the rank.  Every thread zeroes its bins for the next pass.
// first: the first pass of a call - n is the sum of all bins, the wanted rank (n - 1) / 2, and the rows of the
// work-groups are reduced.  last: 1 - the prefix is the median: into the state, and the second selection starts from an
// empty prefix and the same rank; 2 - the prefix is the MAD: the 8 stats are written.
__global__ void __launch_bounds__(1024)
    noise_scan_kernel(int shift, int width, int first, int last, int nrows, NoiseState *st, u64 *bins, const u64 *rows,
                      double *stats)
{
#pragma clang fp contract(off)
    __shared__ u64 wsum[16];
    __shared__ u64 red[3][16];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    // (the state is read by every thread before the barrier below and written by one thread after it)
    const u64 n0 = first ? 0 : st->n, rank0 = first ? 0 : st->rank, prefix0 = first ? 0 : st->prefix;
    if (!first && n0 == 0) return;
    constexpr int PER = (1 << NOISE_MAX_BITS) / 1024;
    const int nb = 1 << width, per = (nb + 1023) / 1024;
    u64 mine[PER];
    u64 sum = 0;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const int i = t * per + j;
        const bool own = j < per && i < nb;
        mine[j] = own ? bins[i] : 0;
        if (own) bins[i] = 0;
        sum += mine[j];
    }
    u64 inc = sum;
    for (int off = 1; off < 64; off <<= 1) {
        const u64 o = __shfl_up(inc, off);
        if (lane >= off) inc += o;
    }
    if (lane == 63) wsum[wave] = inc;
    if (first) {
        u64 kmin = ~(u64)0, kmax = 0, skipped = 0;
        for (int r = t; r < nrows; r += 1024) {
            kmin = rows[3 * r] < kmin ? rows[3 * r] : kmin;
            kmax = rows[3 * r + 1] > kmax ? rows[3 * r + 1] : kmax;
            skipped += rows[3 * r + 2];
        }
        for (int off = 32; off > 0; off >>= 1) {
            const u64 a = __shfl_down(kmin, off), b = __shfl_down(kmax, off);
            kmin = a < kmin ? a : kmin;
            kmax = b > kmax ? b : kmax;
            skipped += __shfl_down(skipped, off);
        }
        if (lane == 0) red[0][wave] = kmin, red[1][wave] = kmax, red[2][wave] = skipped;
    }
    __syncthreads();
    u64 before = 0, total = 0;
    for (int w = 0; w < 16; ++w) {
        if (w < wave) before += wsum[w];
        total += wsum[w];
    }
    const u64 exc = before + inc - sum;
    if (first && t == 0) {
        u64 kmin = red[0][0], kmax = red[1][0], skipped = red[2][0];
        for (int w = 1; w < 16; ++w) {
            kmin = red[0][w] < kmin ? red[0][w] : kmin;
            kmax = red[1][w] > kmax ? red[1][w] : kmax;
            skipped += red[2][w];
        }
        st->n = total;
        st->kmin = kmin;
        st->kmax = kmax;
        st->skipped = skipped;
        if (total == 0 && stats) {
            const double nan = __builtin_nan("");
            stats[0] = 0.0;
            stats[1] = stats[2] = stats[3] = stats[4] = stats[5] = nan;
            stats[6] = (double)skipped;
            stats[7] = 0.0;
        }
    }
    if (first && total == 0) return;
    const u64 rank = first ? (total - 1) / 2 : rank0;
    if (!(sum > 0 && rank >= exc && rank < exc + sum)) return;  // (exactly one thread goes on)
    u64 below = exc;
    int d = -1;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        if (d < 0 && rank < below + mine[j]) d = t * per + j;
        if (d < 0) below += mine[j];
    }
    const u64 prefix = prefix0 | ((u64)d << shift);
    const u64 n = first ? total : n0;
    if (last == 0) {
        st->prefix = prefix;
        st->rank = rank - below;
    } else if (last == 1) {
        st->median = ordered_value(prefix);
        st->prefix = 0;
        st->rank = (n - 1) / 2;
    } else if (stats) {
        const double mad = ordered_value(prefix);
        stats[0] = (double)n;
        stats[1] = st->median;
        stats[2] = mad;
        stats[3] = 1.4826 * mad;
        stats[4] = ordered_value(st->kmin);
        stats[5] = ordered_value(st->kmax);
        stats[6] = (double)st->skipped;
        stats[7] = 0.0;
    }
}

}  // namespace

int image_stats_check(gridhip_ctx *ctx, int64_t N, const double *image, const uint8_t *mask, int64_t border,
                      const double *stats)
{
    if (N < 1 || border < 0 || 2 * border >= N || !image || !stats) return fail(ctx, GRIDHIP_EINVAL, "image_stats: bad argument");
    if (N > CLEAN_MAX_N) return fail(ctx, GRIDHIP_EUNSUPPORTED, "image_stats: N above %lld", (long long)CLEAN_MAX_N);
    const size_t cells = (size_t)N * N;
    if (overlap(mask, cells, image, cells * 8) || overlap(stats, 64, mask, cells) || overlap(stats, 64, image, cells * 8))
        return fail(ctx, GRIDHIP_EINVAL, "image_stats: image, mask and stats must not overlap");
    return GRIDHIP_OK;
}

size_t image_stats_scratch_bytes(gridhip_ctx *ctx) { return layout(ctx).total; }

int image_stats_run(gridhip_ctx *ctx, int64_t N, const double *image, const uint8_t *mask, int64_t border, double *stats,
                    void *scratch)
{
    const NoiseLayout l = layout(ctx);
    char *base = reinterpret_cast<char *>(scratch);
    NoiseState *st = reinterpret_cast<NoiseState *>(base);
    u64 *bins = reinterpret_cast<u64 *>(base + l.state);
    u64 *rows = reinterpret_cast<u64 *>(base + l.state + l.bins);
    const int bits = ctx->img->noise_bits == 8 ? 8 : NOISE_MAX_BITS;
    const int P = (64 + bits - 1) / bits;
    int64_t nwg = (N * N + 1023) / 1024;
    if (nwg > l.nwg) nwg = l.nwg;
    const dim3 grid((unsigned)nwg);
    hipLaunchKernelGGL(noise_init_kernel, dim3(8), dim3(256), 0, ctx->stream, st, bins, 1 << NOISE_MAX_BITS);
    for (int sel = 0; sel < 2; ++sel) {
        for (int p = 0; p < P; ++p) {
            const int top = 64 - bits * p, shift = top > bits ? top - bits : 0, width = top - shift;
            const size_t lds = (size_t)4 << width;
            const int first = sel == 0 && p == 0, last = p == P - 1 ? sel + 1 : 0;
            if (first)
                hipLaunchKernelGGL(noise_hist_kernel<0>, grid, dim3(256), lds, ctx->stream, N, border, image, mask, shift, width,
                                   (const NoiseState *)st, bins, rows);
            else if (sel == 0)
                hipLaunchKernelGGL(noise_hist_kernel<1>, grid, dim3(256), lds, ctx->stream, N, border, image, mask, shift, width,
                                   (const NoiseState *)st, bins, rows);
            else
                hipLaunchKernelGGL(noise_hist_kernel<2>, grid, dim3(256), lds, ctx->stream, N, border, image, mask, shift, width,
                                   (const NoiseState *)st, bins, rows);
            hipLaunchKernelGGL(noise_scan_kernel, dim3(1), dim3(1024), 0, ctx->stream, shift, width, first, last, (int)nwg, st,
                               bins, (const u64 *)rows, stats);
        }
    }
    GH_CHECK_HIP(ctx, hipGetLastError());
    return GRIDHIP_OK;
}

}  // namespace gridhip

using namespace gridhip;

namespace {

int image_stats_any(gridhip_ctx *ctx, bool dev, int64_t N, const double *image, const uint8_t *mask, int64_t border,
                    double *stats)
{
    if (!ctx) return GRIDHIP_EINVAL;
    GH_CHECK(image_stats_check(ctx, N, image, mask, border, stats));
    GH_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    DevBuf scratch;
    GH_CHECK(scratch.alloc(ctx, image_stats_scratch_bytes(ctx)));
    const size_t cells = (size_t)N * N;
    Staged st(ctx, dev);
    image = st.in(image, cells * 8), mask = st.in(mask, cells), stats = st.out(stats, 64);
    GH_CHECK(st.status());
    GH_CHECK(image_stats_run(ctx, N, image, mask, border, stats, scratch.p));
    return st.finish();
}

}  // namespace

extern "C" {

int gridhip_image_stats(gridhip_ctx *ctx, int64_t N, const double *image, const uint8_t *mask, int64_t border,
                        double *stats)
{
    return image_stats_any(ctx, false, N, image, mask, border, stats);
}

int gridhip_image_stats_dev(gridhip_ctx *ctx, int64_t N, const double *image, const uint8_t *mask, int64_t border,
                            double *stats)
{
    return image_stats_any(ctx, true, N, image, mask, border, stats);
}

}  // extern "C"
