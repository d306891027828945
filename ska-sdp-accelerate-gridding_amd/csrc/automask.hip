// Auto-masking (include/gridhip.h, "auto-masking"): the clean mask of a major cycle from the map it is about to clean -
// two levels, the islands above the higher one pruned by size, kept with the whole island above the lower level they lie
// in, grown, and OR-ed into the caller's mask - all on the device, read-back free.
//
// The new piece is connected-component labelling (8-connectivity) by UNION-FIND, a fixed pass structure:
//     am_local_kernel    one work-group per AM_TH x AM_TW tile: label = own index inside the set, AM_NONE outside (each
//                        cell starts at the first cell of its horizontal run, from the rows' ballot masks), the runs
//                        merged with the row above in LDS (32-bit atomicMin on roots), flattened, the tile's component
//                        sizes counted in LDS at the tile-local roots, and written as global cell indices
//     am_border_kernel   one work-group per tile: the cells of its top row and of its left and right columns are merged
//                        with their W, NW, N, NE neighbours that lie in ANOTHER tile, in global memory.  Every adjacent
//                        pair of cells in different tiles is such a (cell, backward neighbour) pair - across an edge, and
//                        across the corner where four tiles meet (NW and NE) alike
//     am_flatten_kernel  label[k] = root(k); a tile-local root that is not the root adds its count to the root's
// THE INVARIANT: label[k] <= k for every cell of the set at every instant, in LDS and in global memory.  It holds after
// the initialisation, and the only write between kernels' boundaries is atomicMin(&label[a], b) with b < a, or a store of
// a root found by following labels, both of which keep it.  Everything terminates because of it:
//   find:   x = label[x] while label[x] != x.  label[x] <= x, so x strictly decreases: at most x steps, whatever other
//           threads write meanwhile (a value read late or stale is a value the cell once had, and that was <= x too).
//   union:  with a > b, old = atomicMin(&label[a], b).  old == a: a was a root and now hangs below b - done.  old < a: a
//           hung below old; it now hangs below min(old, b), and what is left is to unite old and b, both < a.  max(a, b)
//           strictly decreases from one round to the next: at most a rounds, again whatever other threads do.
// No loop waits for another thread, work-group or launch; nothing depends on how many work-groups are resident.  A link
// always goes from the larger index to the smaller, so a component's root is its smallest cell index: the labels after
// the flatten are a function of the set alone.
// Loads of labels that other work-groups change within a launch (the border and flatten kernels) are relaxed agent-scope
// atomic loads: they are served past the CU's L1, which other CUs' stores never refresh.
//
// One call is 13 launches whatever the image holds (the first 11 are automask_label_run, which sources.hip shares):
//     am_peak_kernel, am_levels_kernel                P = max v over the cells that take part; T_hi, T_lo; the counters zeroed
//     local, border, flatten  at T_hi                 components of H and their sizes (plane A: labels, plane B: sizes)
//     am_seeds_kernel                                 bytes: 1 on the cells of components with >= min_cells cells
//     local, border, flatten  at T_lo                 components of L (plane B: labels; plane A, zeroed: kept flags)
//     am_mark_kernel, am_keep_kernel                  a component of L that holds a seed is flagged; bytes: 1 on K
//     am_grow_kernel                                  LDS tile with a halo of `grow` cells; OR into the mask
//     am_stats_kernel                                 the 8 stats
// There is no floating-point atomic: levels are compared, never summed; counts are 32-bit integers (N <= 46340), added
// per work-group after a reduction in the work-group.  An early end (reason 2, 3) is decided by am_levels_kernel, which
// then writes the stats; every later kernel reads the reason and leaves.
#include "common.h"
#include "imaging.h"

namespace gridhip {

namespace {

typedef unsigned long long u64;

constexpr int AM_TH = 32, AM_TW = 32;  // the labelling tile (tests/test_gpu_automask.py reads these two numbers)
constexpr int AM_CELLS = AM_TH * AM_TW, AM_PER = AM_CELLS / 256;
constexpr int AM_NONE = -1;  // the label of a cell outside the set
constexpr int64_t AM_MAX_N = 46340, AM_MAX_GROW = 32;
constexpr u64 AM_EXP = 0x7ff0000000000000ULL;
static_assert(AM_TW == 32 && AM_TH % 8 == 0, "a wave's ballot holds two rows of a tile");

// (AmState, the head of the scratch block, is in imaging.h: sources.hip reads the levels and the reason from it)
struct AmLayout {
    size_t state, rows, planeA, planeB, bytes, total;
    int nwg;
};

AmLayout layout(gridhip_ctx *ctx, int64_t N)
{
    AmLayout l;
    const size_t cells = (size_t)N * N;
    l.nwg = ctx->num_cu * 4;
    l.state = 0;
    l.rows = 256;
    l.planeA = l.rows + (((size_t)l.nwg * 16 + 255) & ~(size_t)255);
    l.planeB = l.planeA + ((cells * 4 + 255) & ~(size_t)255);
    l.bytes = l.planeB + ((cells * 4 + 255) & ~(size_t)255);
    l.total = l.bytes + ((cells + 255) & ~(size_t)255);
    return l;
}

__device__ __forceinline__ bool takes_part(int64_t N, int64_t border, int64_t y, int64_t x, double v)
{
    return y >= border && y < N - border && x >= border && x < N - border &&
           (__builtin_bit_cast(u64, v) & AM_EXP) != AM_EXP;
}

// the sum of c over the work-group in thread 0 (sh: one slot per wave)
__device__ __forceinline__ unsigned int group_sum(unsigned int c, unsigned int *sh)
{
    for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off);
    const int wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
    if ((threadIdx.x & 63) == 0) sh[wave] = c;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < nwaves; ++w) c += sh[w];
    return c;
}

// rows[2 b] = the largest key of v over the cells of work-group b that take part, rows[2 b + 1] = whether it has any
__global__ void __launch_bounds__(256)
    am_peak_kernel(int64_t N, int64_t border, const double *__restrict__ image, int absolute, u64 *__restrict__ rows)
{
    __shared__ u64 sh[2][4];
    const int64_t cells = N * N, T = (int64_t)gridDim.x * 256;
    const int64_t sy = T / N, sx = T % N;
    int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int64_t y = k / N, x = k % N;
    u64 kmax = 0, any = 0;
    for (; k < cells; k += T) {
        if (y >= border && y < N - border && x >= border && x < N - border) {
            const double v = image[k];
            if ((__builtin_bit_cast(u64, v) & AM_EXP) != AM_EXP) {
                const u64 key = ordered_bits(absolute ? fabs(v) : v);
                kmax = key > kmax ? key : kmax;
                any = 1;
            }
        }
        y += sy, x += sx;
        if (x >= N) x -= N, y += 1;
    }
    for (int off = 32; off > 0; off >>= 1) {
        const u64 a = __shfl_down(kmax, off);
        kmax = a > kmax ? a : kmax;
        any |= __shfl_down(any, off);
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) sh[0][wave] = kmax, sh[1][wave] = any;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) {
            kmax = sh[0][w] > kmax ? sh[0][w] : kmax;
            any |= sh[1][w];
        }
        rows[2 * blockIdx.x] = kmax;
        rows[2 * blockIdx.x + 1] = any;
    }
}

// One work-group: P from the rows; T_hi and T_lo, each product rounded once; the counters zeroed; reason 3 (an nsigma term
// is wanted and sigma is NaN) or 2 (no cell takes part) ends the call here, with the stats written.
__global__ void __launch_bounds__(256)
    am_levels_kernel(int nrows, const u64 *__restrict__ rows, double thr_hi, double thr_lo, double nsigma_hi,
                     double nsigma_lo, const double *noise, double peak_frac, AmState *st, double *stats)
{
#pragma clang fp contract(off)
    __shared__ u64 sh[2][4];
    u64 kmax = 0, any = 0;
    for (int r = threadIdx.x; r < nrows; r += 256) {
        kmax = rows[2 * r] > kmax ? rows[2 * r] : kmax;
        any |= rows[2 * r + 1];
    }
    for (int off = 32; off > 0; off >>= 1) {
        const u64 a = __shfl_down(kmax, off);
        kmax = a > kmax ? a : kmax;
        any |= __shfl_down(any, off);
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) sh[0][wave] = kmax, sh[1][wave] = any;
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int w = 1; w < 4; ++w) {
        kmax = sh[0][w] > kmax ? sh[0][w] : kmax;
        any |= sh[1][w];
    }
    const double nan = __builtin_nan("");
    const double P = any ? ordered_value(kmax) : nan;
    double T_hi = thr_hi, T_lo = thr_lo;
    int reason = 0;
    if (nsigma_hi > 0.0) {
        const double sigma = *noise;
        if (sigma != sigma) {
            reason = 3;
            T_hi = T_lo = nan;
        } else {
            const double a = nsigma_hi * sigma;
            T_hi = a > T_hi ? a : T_hi;
            if (nsigma_lo > 0.0) {
                const double b = nsigma_lo * sigma;
                T_lo = b > T_lo ? b : T_lo;
            }
        }
    }
    if (reason == 0 && !any) reason = 2;
    if (reason == 0 && peak_frac > 0.0) {
        const double c = peak_frac * P;
        T_hi = c > T_hi ? c : T_hi;
        T_lo = c > T_lo ? c : T_lo;
    }
    st->T_hi = T_hi;
    st->T_lo = T_lo;
    st->P = P;
    st->reason = reason;
    st->nH = st->nSurv = st->nKept = st->nNew = 0;
    if (reason != 0) {
        stats[0] = T_hi;
        stats[1] = T_lo;
        stats[2] = P;
        stats[3] = stats[4] = stats[5] = stats[6] = 0.0;
        stats[7] = (double)reason;
    }
}

// ---- union-find: the same two functions over a tile's labels in LDS and over the image's in global memory ---------------
__device__ __forceinline__ int lds_load(const int *lab, int x)
{
    return __hip_atomic_load(&lab[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ int dev_load(const int *lab, int x)
{
    return __hip_atomic_load(&lab[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// x is a cell of the set.  Terminates: label[x] <= x (the invariant), so x strictly decreases until label[x] == x.
template <bool LDS>
__device__ __forceinline__ int am_find(const int *lab, int x)
{
    for (;;) {
        const int p = LDS ? lds_load(lab, x) : dev_load(lab, x);
        if (p >= x || p < 0) return x;  // p == x: a root.  (p > x or p < 0 cannot be: they would end the loop, never extend it)
        x = p;
    }
}

// a and b are cells of the set.  Terminates: every round but the last replaces the larger of the two by a smaller index.
template <bool LDS>
__device__ __forceinline__ void am_union(int *lab, int a, int b)
{
    for (;;) {
        a = am_find<LDS>(lab, a);
        b = am_find<LDS>(lab, b);
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = atomicMin(&lab[a], b);  // the link goes from the larger index to the smaller
        if (old >= a) return;                   // a was a root (old == a; more cannot be)
        a = old;                                // a hung below old < a: old and b are left to unite
    }
}

// One tile.  Thread t takes the cells (ly, lx) = ((t >> 5) + 8 j, t & 31), j = 0 .. 3: a wave holds two rows, and its
// ballot their two 32-bit masks.  lo: the set is v > T_lo (else v > T_hi).  aux receives the tile-local component sizes at
// the tile-local roots and 0 elsewhere (count), or 0 everywhere.
__global__ void __launch_bounds__(256)
    am_local_kernel(int64_t N, int64_t border, const double *__restrict__ image, int absolute, int lo, int count,
                    const AmState *st, int *__restrict__ label, int *__restrict__ aux)
{
    __shared__ int lab[AM_CELLS];
    __shared__ int cnt[AM_CELLS];
    __shared__ unsigned int rowmask[AM_TH];
    if (st->reason != 0) return;
    const double T = lo ? st->T_lo : st->T_hi;
    const int64_t y0 = (int64_t)blockIdx.y * AM_TH, x0 = (int64_t)blockIdx.x * AM_TW;
    const int lx = threadIdx.x & 31, lr = threadIdx.x >> 5;
    bool in[AM_PER];
#pragma unroll
    for (int j = 0; j < AM_PER; ++j) {
        const int ly = lr + 8 * j;
        const int64_t y = y0 + ly, x = x0 + lx;
        in[j] = false;
        if (y < N && x < N) {
            const double raw = image[y * N + x];
            const double v = absolute ? fabs(raw) : raw;
            in[j] = takes_part(N, border, y, x, raw) && v > T;
        }
        const u64 b = __ballot(in[j]);
        if (lx == 0) rowmask[ly] = (threadIdx.x & 32) ? (unsigned int)(b >> 32) : (unsigned int)b;
    }
    __syncthreads();
    // the first cell of the horizontal run: one past the nearest cell to the left that is outside the set
#pragma unroll
    for (int j = 0; j < AM_PER; ++j) {
        const int ly = lr + 8 * j, i = ly * AM_TW + lx;
        const unsigned int out_left = ~rowmask[ly] & ((1u << lx) - 1u);
        const int start = out_left ? 32 - __clz(out_left) : 0;
        lab[i] = in[j] ? ly * AM_TW + start : AM_NONE;
        cnt[i] = 0;
    }
    __syncthreads();
    // the row above: N if it is in the set (NW and NE then lie in N's run), else NW and NE each
#pragma unroll
    for (int j = 0; j < AM_PER; ++j) {
        const int ly = lr + 8 * j, i = ly * AM_TW + lx;
        if (!in[j] || ly == 0) continue;
        const unsigned int up = rowmask[ly - 1];
        const int above = (ly - 1) * AM_TW + lx;
        if ((up >> lx) & 1u) {
            am_union<true>(lab, i, above);
        } else {
            if (lx > 0 && ((up >> (lx - 1)) & 1u)) am_union<true>(lab, i, above - 1);
            if (lx < AM_TW - 1 && ((up >> (lx + 1)) & 1u)) am_union<true>(lab, i, above + 1);
        }
    }
    __syncthreads();
    int root[AM_PER];
#pragma unroll
    for (int j = 0; j < AM_PER; ++j) {
        const int i = (lr + 8 * j) * AM_TW + lx;
        root[j] = in[j] ? am_find<true>(lab, i) : AM_NONE;
        if (in[j] && count) atomicAdd(&cnt[root[j]], 1);
    }
    __syncthreads();
    // a tile-local index and the global one order the cells of a tile alike: the smallest stays the smallest
#pragma unroll
    for (int j = 0; j < AM_PER; ++j) {
        const int ly = lr + 8 * j, i = ly * AM_TW + lx;
        const int64_t y = y0 + ly, x = x0 + lx;
        if (y < N && x < N) {
            const int64_t k = y * N + x;
            const int r = root[j];
            label[k] = in[j] ? (int)((y0 + r / AM_TW) * N + x0 + r % AM_TW) : AM_NONE;
            aux[k] = in[j] && r == i ? cnt[i] : 0;
        }
    }
}

// One tile, 128 threads of which 96 work: thread t < 32 takes the cell t of the top row, t < 64 the cell t - 32 of the
// left column, t < 96 the cell t - 64 of the right column (a corner cell is taken twice, which unites it twice).
__global__ void __launch_bounds__(128) am_border_kernel(int64_t N, const AmState *st, int *label)
{
    if (st->reason != 0) return;
    const int t = threadIdx.x;
    if (t >= 96) return;
    const int ly = t < 32 ? 0 : (t & 31), lx = t < 32 ? t : (t < 64 ? 0 : AM_TW - 1);
    const int64_t y = (int64_t)blockIdx.y * AM_TH + ly, x = (int64_t)blockIdx.x * AM_TW + lx;
    if (y >= N || x >= N) return;
    const int64_t k = y * N + x;
    if (label[k] == AM_NONE) return;  // (whether a cell is in the set never changes in this launch)
    const int dy[4] = {0, -1, -1, -1}, dx[4] = {-1, -1, 0, 1};
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        const int64_t ey = y + dy[d], ex = x + dx[d];
        if (ey < 0 || ex < 0 || ex >= N) continue;
        if (ey / AM_TH == y / AM_TH && ex / AM_TW == x / AM_TW) continue;  // the same tile: united in LDS already
        const int64_t e = ey * N + ex;
        if (label[e] == AM_NONE) continue;
        am_union<false>(label, (int)k, (int)e);
    }
}

// label[k] = root(k).  count: a cell that carries a tile-local size and is not the root adds it to the root's - one
// integer atomic per (tile, component), never one per cell; *ncomp += the roots.
__global__ void __launch_bounds__(256)
    am_flatten_kernel(int64_t cells, const AmState *st, int *label, int *aux, int count, unsigned int *ncomp)
{
    __shared__ unsigned int sh[4];
    if (st->reason != 0) return;
    unsigned int roots = 0;
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < cells; k += (int64_t)gridDim.x * 256) {
        if (dev_load(label, (int)k) == AM_NONE) continue;
        const int r = am_find<false>(label, (int)k);
        __hip_atomic_store(&label[k], r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // r <= k: the invariant holds
        if (r == (int)k) {
            roots += 1;
        } else if (count) {
            const int c = aux[k];  // (written by the local kernel; only roots' cells are added to in this launch)
            if (c > 0) atomicAdd(&aux[r], c);
        }
    }
    roots = group_sum(roots, sh);
    if (ncomp && threadIdx.x == 0 && roots) atomicAdd(ncomp, roots);
}

// seed[k] = the cell lies in a component of H with at least min_cells cells
__global__ void __launch_bounds__(256)
    am_seeds_kernel(int64_t cells, int64_t min_cells, AmState *st, const int *__restrict__ label,
                    const int *__restrict__ size, uint8_t *__restrict__ seed)
{
    __shared__ unsigned int sh[4];
    if (st->reason != 0) return;
    unsigned int surv = 0;
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < cells; k += (int64_t)gridDim.x * 256) {
        const int r = label[k];
        const bool s = r != AM_NONE && (int64_t)size[r] >= min_cells;
        seed[k] = s ? 1 : 0;
        if (s && r == (int)k) surv += 1;
    }
    surv = group_sum(surv, sh);
    if (threadIdx.x == 0 && surv) atomicAdd(&st->nSurv, surv);
}

// keep[root of L's component] = 1 where the component holds a seed (every writer stores the same 1)
__global__ void __launch_bounds__(256)
    am_mark_kernel(int64_t cells, const AmState *st, const int *__restrict__ label, const uint8_t *__restrict__ seed,
                   int *keep)
{
    if (st->reason != 0) return;
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < cells; k += (int64_t)gridDim.x * 256) {
        const int r = label[k];
        if (seed[k] && r != AM_NONE) keep[r] = 1;
    }
}

// kbyte[k] = the cell lies in a kept component of L
__global__ void __launch_bounds__(256)
    am_keep_kernel(int64_t cells, AmState *st, const int *__restrict__ label, const int *__restrict__ keep,
                   uint8_t *__restrict__ kbyte)
{
    __shared__ unsigned int sh[4];
    if (st->reason != 0) return;
    unsigned int kept = 0;
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < cells; k += (int64_t)gridDim.x * 256) {
        const int r = label[k];
        const bool in = r != AM_NONE && keep[r] != 0;
        kbyte[k] = in ? 1 : 0;
        if (in && r == (int)k) kept += 1;
    }
    kept = group_sum(kept, sh);
    if (threadIdx.x == 0 && kept) atomicAdd(&st->nKept, kept);
}

// One AM_TH x AM_TW tile of the mask.  The bytes of K over the tile and a halo of g cells go to LDS (0 outside the image),
// each row is OR-ed over the window of 2 g + 1 columns, then each column over 2 g + 1 rows: the cells within Chebyshev
// distance g of K.  A cell of the border region that is reached and whose mask byte is 0 becomes 1; nothing else is written.
// dynamic LDS: (AM_TH + 2 g) * (AM_TW + 2 g) + (AM_TH + 2 g) * AM_TW bytes
__global__ void __launch_bounds__(256)
    am_grow_kernel(int64_t N, int64_t border, int g, AmState *st, const uint8_t *__restrict__ kbyte,
                   uint8_t *__restrict__ mask)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t am_lds[];
    __shared__ unsigned int sh[4];
    if (st->reason != 0) return;
    const int H = AM_TH + 2 * g, W = AM_TW + 2 * g;
    uint8_t *src = am_lds, *row = am_lds + H * W;
    const int64_t y0 = (int64_t)blockIdx.y * AM_TH, x0 = (int64_t)blockIdx.x * AM_TW;
    for (int i = threadIdx.x; i < H * W; i += 256) {
        const int64_t y = y0 - g + i / W, x = x0 - g + i % W;
        src[i] = (y >= 0 && y < N && x >= 0 && x < N) ? kbyte[y * N + x] : 0;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < H * AM_TW; i += 256) {
        const uint8_t *p = src + (i / AM_TW) * W + i % AM_TW;
        uint8_t any = 0;
        for (int d = 0; d <= 2 * g; ++d) any |= p[d];
        row[i] = any;
    }
    __syncthreads();
    unsigned int fresh = 0;
    for (int i = threadIdx.x; i < AM_CELLS; i += 256) {
        const int ly = i / AM_TW, lx = i % AM_TW;
        const int64_t y = y0 + ly, x = x0 + lx;
        if (!(y >= border && y < N - border && x >= border && x < N - border)) continue;
        uint8_t any = 0;
        for (int d = 0; d <= 2 * g; ++d) any |= row[(ly + d) * AM_TW + lx];
        if (any && mask[y * N + x] == 0) {
            mask[y * N + x] = 1;
            fresh += 1;
        }
    }
    fresh = group_sum(fresh, sh);
    if (threadIdx.x == 0 && fresh) atomicAdd(&st->nNew, fresh);
}

__global__ void am_stats_kernel(const AmState *st, double *stats)
{
    if (st->reason != 0) return;  // (am_levels_kernel wrote them)
    stats[0] = st->T_hi;
    stats[1] = st->T_lo;
    stats[2] = st->P;
    stats[3] = (double)st->nH;
    stats[4] = (double)st->nSurv;
    stats[5] = (double)st->nKept;
    stats[6] = (double)st->nNew;
    stats[7] = 0.0;
}

bool level_ok(double x) { return x >= 0.0 && x < __builtin_inf(); }

}  // namespace

int automask_check(gridhip_ctx *ctx, int64_t N, const double *image, const uint8_t *mask, int64_t border, double thr_hi,
                   double thr_lo, double nsigma_hi, double nsigma_lo, const double *noise, double peak_frac,
                   int64_t min_cells, int64_t grow, const double *stats)
{
    if (!mask || !stats || grow < 0) return fail(ctx, GRIDHIP_EINVAL, "automask: bad argument");
    GH_CHECK(automask_levels_check(ctx, "automask", N, image, border, thr_hi, thr_lo, nsigma_hi, nsigma_lo, noise, peak_frac,
                                   min_cells));
    if (N <= AM_MAX_N) {  // (above it the call is refused below, and the byte counts are not needed)
        const size_t cells = (size_t)N * N;
        if (overlap(mask, cells, image, cells * 8) || overlap(stats, 64, image, cells * 8) ||
            overlap(stats, 64, mask, cells))
            return fail(ctx, GRIDHIP_EINVAL, "automask: image, mask and stats must not overlap");
    }
    if (grow > AM_MAX_GROW) return fail(ctx, GRIDHIP_EUNSUPPORTED, "automask: grow above %d", (int)AM_MAX_GROW);
    if (N > AM_MAX_N) return fail(ctx, GRIDHIP_EUNSUPPORTED, "automask: N above %d", (int)AM_MAX_N);
    return GRIDHIP_OK;
}

size_t automask_scratch_bytes(gridhip_ctx *ctx, int64_t N) { return layout(ctx, N).total; }

int automask_levels_check(gridhip_ctx *ctx, const char *who, int64_t N, const double *image, int64_t border, double thr_hi,
                          double thr_lo, double nsigma_hi, double nsigma_lo, const double *noise, double peak_frac,
                          int64_t min_cells)
{
    if (N < 1 || border < 0 || 2 * border >= N || !image || min_cells < 1)
        return fail(ctx, GRIDHIP_EINVAL, "%s: bad argument", who);
    if (!level_ok(thr_hi) || !level_ok(thr_lo) || !level_ok(nsigma_hi) || !level_ok(nsigma_lo) || thr_lo > thr_hi ||
        nsigma_lo > nsigma_hi || !(peak_frac >= 0.0 && peak_frac < 1.0) || (nsigma_hi > 0.0 && !noise))
        return fail(ctx, GRIDHIP_EINVAL, "%s: bad thr, nsigma, noise or peak_frac", who);
    return GRIDHIP_OK;
}

AmPlanes automask_planes(gridhip_ctx *ctx, int64_t N, void *scratch)
{
    const AmLayout l = layout(ctx, N);
    char *base = reinterpret_cast<char *>(scratch);
    return AmPlanes{reinterpret_cast<AmState *>(base + l.state), reinterpret_cast<int *>(base + l.planeB),
                    reinterpret_cast<int *>(base + l.planeA), reinterpret_cast<uint8_t *>(base + l.bytes)};
}

int automask_label_run(gridhip_ctx *ctx, int64_t N, const double *image, int64_t border, int absolute, double thr_hi,
                       double thr_lo, double nsigma_hi, double nsigma_lo, const double *noise, double peak_frac,
                       int64_t min_cells, double *stats, void *scratch)
{
    const AmLayout l = layout(ctx, N);
    char *base = reinterpret_cast<char *>(scratch);
    AmState *st = reinterpret_cast<AmState *>(base + l.state);
    u64 *rows = reinterpret_cast<u64 *>(base + l.rows);
    int *A = reinterpret_cast<int *>(base + l.planeA), *B = reinterpret_cast<int *>(base + l.planeB);
    uint8_t *bytes = reinterpret_cast<uint8_t *>(base + l.bytes);
    const int64_t cells = N * N;
    int64_t nwg = (cells + 1023) / 1024;
    if (nwg > l.nwg) nwg = l.nwg;
    const dim3 tiles((unsigned)((N + AM_TW - 1) / AM_TW), (unsigned)((N + AM_TH - 1) / AM_TH));  // at most 1449 x 1449
    const dim3 flat = grid_for(ctx, cells);
    hipStream_t s = ctx->stream;
    absolute = absolute != 0;
    hipLaunchKernelGGL(am_peak_kernel, dim3((unsigned)nwg), dim3(256), 0, s, N, border, image, absolute, rows);
    hipLaunchKernelGGL(am_levels_kernel, dim3(1), dim3(256), 0, s, (int)nwg, (const u64 *)rows, thr_hi, thr_lo, nsigma_hi,
                       nsigma_lo, noise, peak_frac, st, stats);
    // H: labels in A, sizes in B
    hipLaunchKernelGGL(am_local_kernel, tiles, dim3(256), 0, s, N, border, image, absolute, 0, 1, (const AmState *)st, A, B);
    hipLaunchKernelGGL(am_border_kernel, tiles, dim3(128), 0, s, N, (const AmState *)st, A);
    hipLaunchKernelGGL(am_flatten_kernel, flat, dim3(256), 0, s, cells, (const AmState *)st, A, B, 1, &st->nH);
    hipLaunchKernelGGL(am_seeds_kernel, flat, dim3(256), 0, s, cells, min_cells, st, (const int *)A, (const int *)B, bytes);
    // L: labels in B, the kept flags in A (zeroed by the local kernel)
    hipLaunchKernelGGL(am_local_kernel, tiles, dim3(256), 0, s, N, border, image, absolute, 1, 0, (const AmState *)st, B, A);
    hipLaunchKernelGGL(am_border_kernel, tiles, dim3(128), 0, s, N, (const AmState *)st, B);
    hipLaunchKernelGGL(am_flatten_kernel, flat, dim3(256), 0, s, cells, (const AmState *)st, B, A, 0, (unsigned int *)nullptr);
    hipLaunchKernelGGL(am_mark_kernel, flat, dim3(256), 0, s, cells, (const AmState *)st, (const int *)B,
                       (const uint8_t *)bytes, A);
    hipLaunchKernelGGL(am_keep_kernel, flat, dim3(256), 0, s, cells, st, (const int *)B, (const int *)A, bytes);
    GH_CHECK_HIP(ctx, hipGetLastError());
    return GRIDHIP_OK;
}

int automask_run(gridhip_ctx *ctx, int64_t N, const double *image, uint8_t *mask, int64_t border, int absolute,
                 double thr_hi, double thr_lo, double nsigma_hi, double nsigma_lo, const double *noise, double peak_frac,
                 int64_t min_cells, int64_t grow, double *stats, void *scratch)
{
    GH_CHECK(automask_label_run(ctx, N, image, border, absolute, thr_hi, thr_lo, nsigma_hi, nsigma_lo, noise, peak_frac,
                                min_cells, stats, scratch));
    const AmPlanes p = automask_planes(ctx, N, scratch);
    const dim3 tiles((unsigned)((N + AM_TW - 1) / AM_TW), (unsigned)((N + AM_TH - 1) / AM_TH));
    hipStream_t s = ctx->stream;
    const int g = (int)grow;
    const size_t lds = (size_t)(AM_TH + 2 * g) * (AM_TW + 2 * g) + (size_t)(AM_TH + 2 * g) * AM_TW;  // at most 12 KB
    hipLaunchKernelGGL(am_grow_kernel, tiles, dim3(256), lds, s, N, border, g, p.state, (const uint8_t *)p.kbyte, mask);
    hipLaunchKernelGGL(am_stats_kernel, dim3(1), dim3(1), 0, s, (const AmState *)p.state, stats);
    GH_CHECK_HIP(ctx, hipGetLastError());
    return GRIDHIP_OK;
}

}  // namespace gridhip

using namespace gridhip;

namespace {

int automask_any(gridhip_ctx *ctx, bool dev, int64_t N, const double *image, uint8_t *mask, int64_t border, int absolute,
                 double thr_hi, double thr_lo, double nsigma_hi, double nsigma_lo, const double *noise, double peak_frac,
                 int64_t min_cells, int64_t grow, double *stats)
{
    if (!ctx) return GRIDHIP_EINVAL;
    GH_CHECK(automask_check(ctx, N, image, mask, border, thr_hi, thr_lo, nsigma_hi, nsigma_lo, noise, peak_frac, min_cells,
                            grow, stats));
    GH_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    DevBuf scratch;
    GH_CHECK(scratch.alloc(ctx, automask_scratch_bytes(ctx, N)));
    const size_t cells = (size_t)N * N;
    Staged st(ctx, dev);
    image = st.in(image, cells * 8), mask = st.inout(mask, mask, cells), noise = st.in(noise, 8), stats = st.out(stats, 64);
    GH_CHECK(st.status());
    GH_CHECK(automask_run(ctx, N, image, mask, border, absolute, thr_hi, thr_lo, nsigma_hi, nsigma_lo, noise, peak_frac,
                          min_cells, grow, stats, scratch.p));
    return st.finish();
}

}  // namespace

extern "C" {

int gridhip_automask(gridhip_ctx *ctx, int64_t N, const double *image, uint8_t *mask, int64_t border, int absolute,
                     double thr_hi, double thr_lo, double nsigma_hi, double nsigma_lo, const double *noise,
                     double peak_frac, int64_t min_cells, int64_t grow, double *stats)
{
    return automask_any(ctx, false, N, image, mask, border, absolute, thr_hi, thr_lo, nsigma_hi, nsigma_lo, noise, peak_frac,
                        min_cells, grow, stats);
}

int gridhip_automask_dev(gridhip_ctx *ctx, int64_t N, const double *image, uint8_t *mask, int64_t border, int absolute,
                         double thr_hi, double thr_lo, double nsigma_hi, double nsigma_lo, const double *noise,
                         double peak_frac, int64_t min_cells, int64_t grow, double *stats)
{
    return automask_any(ctx, true, N, image, mask, border, absolute, thr_hi, thr_lo, nsigma_hi, nsigma_lo, noise, peak_frac,
                        min_cells, grow, stats);
}

}  // extern "C"
