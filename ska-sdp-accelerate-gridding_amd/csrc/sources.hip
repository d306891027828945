// Source finding (include/gridhip.h, "source finding"): from a map to a catalogue - the islands of auto-masking's steps
// 1-3, each measured by its moments and written as one row of a component list that gridhip_dft_predict takes as it is -
// all on the device, read-back free.
//
// The labelling is automask.hip's (automask_label_run: 11 launches).  It leaves the labels of L in one int32 plane - a
// cell's label is the smallest index of its component - the bytes of K, and a second int32 plane that is free again.
// An island's ROOT is the cell with label[k] == k that lies in K.  Then, whatever the image holds:
//     src_count_kernel    the roots of segments of CFI_SEG = 1024 cells are counted (dft.hip's compaction: per-segment
//     (segment_scan)      counts, one work-group scans them, *count = the islands found)
//     src_scatter_kernel  recounts its segment, ranks its roots by a scan over the work-group: the root at rank r is row r
//                         - ascending label order.  spare[root] = r; a row below max_c gets its root and a box of that
//                         one cell
//     src_box_kernel      one flat pass over K: a cell finds its row through spare[label[k]] and widens the row's box by
//                         32-bit integer atomicMin / atomicMax - exact, whatever the order.  A wave whose 64 cells all
//                         belong to one row (the inside of any island wider than a wave) reduces its four bounds by
//                         shuffles first and sends one lane; a bound the box already holds is not sent at all (a box
//                         only widens, so a stale read can only cost an atomic, never lose one)
//     src_measure_kernel  one work-group of 256 threads per row.  It walks the row's box in row-major order, thread t
//                         the cells t, t + 256, ..., and keeps those whose label is the row's root: nested and
//                         interleaved boxes read each other's cells and drop them.  Walk 1: the peak by image_stats' key,
//                         the smaller index among equals.  Walk 2: the count and the six sums about the peak's cell, each
//                         term one rounded product of the value and an exact integer.  Both are reduced by a wave shuffle
//                         tree and then a fixed tree over the four waves in LDS.  Thread 0 derives the fields and writes
//                         the rows.
//     src_stats_kernel    one thread: the 8 stats; the fluxes are added in row order
// DETERMINISM.  A thread's partial sum runs over its cells in walk order, the trees are fixed, and which cells a thread
// takes depends on the box alone: the sums are a function of the image.  There is no floating-point atomic anywhere.
// An island whose box is huge is walked by one work-group - see DESIGN.md §9 for what that costs.
// DEBLENDING (the option "sources_deblend" = r > 0) puts six launches in front of src_count_kernel that turn the labels
// into `sub`, the peak each cell of K climbs to (below, "deblending"); the kernels above then run on sub as they are, on
// roots that are peaks, and src_measure_kernel takes the island's label and its peak count for the info row.  With the
// option at 0 none of it is launched and no scratch is drawn for it.
#include "common.h"
#include "imaging.h"

namespace gridhip {

namespace {

typedef unsigned long long u64;

constexpr int SRC_INFO = GRIDHIP_SRC_DOUBLES;
static_assert(SRC_INFO == 16, "an info row is 16 doubles");

struct SrcLayout {
    size_t segcount, offs, roots, boxes, total;
    int64_t nseg;
};

SrcLayout layout(int64_t N, int64_t max_c)
{
    SrcLayout l;
    l.nseg = (N * N + CFI_SEG - 1) / CFI_SEG;
    l.segcount = 0;
    l.offs = ((size_t)l.nseg * 4 + 255) & ~(size_t)255;
    l.roots = l.offs + (((size_t)l.nseg * 8 + 255) & ~(size_t)255);
    l.boxes = l.roots + (((size_t)max_c * 4 + 255) & ~(size_t)255);
    l.total = l.boxes + (((size_t)max_c * 16 + 255) & ~(size_t)255);
    return l;
}

__device__ __forceinline__ bool is_root(const int *__restrict__ label, const uint8_t *__restrict__ kbyte, int64_t cells,
                                        int64_t e)
{
    return e < cells && kbyte[e] != 0 && label[e] == (int)e;
}

__global__ void __launch_bounds__(256)
    src_count_kernel(int64_t cells, const AmState *st, const int *__restrict__ label, const uint8_t *__restrict__ kbyte,
                     int64_t nseg, unsigned int *__restrict__ segcount)
{
    __shared__ unsigned int lds[4];
    const bool run = st->reason == 0;  // (an early end left the planes as an earlier call had them: no island)
    for (int64_t seg = blockIdx.x; seg < nseg; seg += gridDim.x) {
        unsigned int mine = 0;
        if (run)
            for (int j = 0; j < 4; ++j) mine += is_root(label, kbyte, cells, seg * CFI_SEG + 4 * threadIdx.x + j);
        unsigned int total;
        block_rank(mine, lds, &total);
        if (threadIdx.x == 0) segcount[seg] = total;
    }
}

// box: { y0, y1, x0, x1 } per row
__global__ void __launch_bounds__(256)
    src_scatter_kernel(int64_t N, const AmState *st, const int *__restrict__ label, const uint8_t *__restrict__ kbyte,
                       int64_t nseg, const int64_t *__restrict__ offs, int64_t max_c, int *__restrict__ spare,
                       int *__restrict__ roots, int *__restrict__ boxes)
{
    __shared__ unsigned int lds[4];
    if (st->reason != 0) return;
    const int64_t cells = N * N;
    for (int64_t seg = blockIdx.x; seg < nseg; seg += gridDim.x) {
        unsigned int mine = 0;
        bool set[4];
        for (int j = 0; j < 4; ++j) {
            set[j] = is_root(label, kbyte, cells, seg * CFI_SEG + 4 * threadIdx.x + j);
            mine += set[j];
        }
        unsigned int total;
        int64_t row = offs[seg] + block_rank(mine, lds, &total);
        for (int j = 0; j < 4; ++j) {
            if (!set[j]) continue;
            const int64_t e = seg * CFI_SEG + 4 * threadIdx.x + j;
            spare[e] = (int)row;  // (fewer islands than cells, and those are below 2^31)
            if (row < max_c) {
                const int y = (int)(e / N), x = (int)(e - (int64_t)y * N);
                roots[row] = (int)e;
                boxes[4 * row + 0] = y, boxes[4 * row + 1] = y, boxes[4 * row + 2] = x, boxes[4 * row + 3] = x;
            }
            ++row;
        }
    }
}

__device__ __forceinline__ int box_load(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// widen box b by the bounds given, sending only what it does not hold already
__device__ __forceinline__ void box_widen(int *b, int ylo, int yhi, int xlo, int xhi)
{
    if (ylo < box_load(b + 0)) atomicMin(b + 0, ylo);
    if (yhi > box_load(b + 1)) atomicMax(b + 1, yhi);
    if (xlo < box_load(b + 2)) atomicMin(b + 2, xlo);
    if (xhi > box_load(b + 3)) atomicMax(b + 3, xhi);
}

__global__ void __launch_bounds__(256)
    src_box_kernel(int64_t N, const AmState *st, const int *__restrict__ label, const uint8_t *__restrict__ kbyte,
                   const int *__restrict__ spare, int64_t max_c, int *boxes)
{
    if (st->reason != 0) return;
    const int64_t cells = N * N, step = (int64_t)gridDim.x * 256;
    for (int64_t base = (int64_t)blockIdx.x * 256; base < cells; base += step) {  // (uniform over the work-group)
        const int64_t k = base + threadIdx.x;
        int row = -1, y = 0, x = 0;
        if (k < cells && kbyte[k] != 0) {
            const int r = spare[label[k]];
            if (r < max_c) {
                row = r;
                y = (int)(k / N), x = (int)(k - (int64_t)y * N);
            }
        }
        const int first = __shfl(row, 0);
        if (__all(row == first)) {  // one row for the whole wave (or none of its cells counts)
            if (first < 0) continue;
            int ylo = y, yhi = y, xlo = x, xhi = x;
            for (int off = 32; off > 0; off >>= 1) {
                const int a = __shfl_down(ylo, off), b = __shfl_down(yhi, off), c = __shfl_down(xlo, off),
                          d = __shfl_down(xhi, off);
                ylo = a < ylo ? a : ylo, yhi = b > yhi ? b : yhi, xlo = c < xlo ? c : xlo, xhi = d > xhi ? d : xhi;
            }
            if ((threadIdx.x & 63) == 0) box_widen(boxes + 4 * (int64_t)first, ylo, yhi, xlo, xhi);
        } else if (row >= 0) {
            box_widen(boxes + 4 * (int64_t)row, y, y, x, x);
        }
    }
}

// the sum of x over the work-group in thread 0: a shuffle tree in each wave, then (w0 + w1) + (w2 + w3); lds: 4 values
__device__ __forceinline__ double tree_sum256(double x, double *lds)
{
    for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o);
    __syncthreads();  // (the last use of lds has been read)
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = x;
    __syncthreads();
    return (lds[0] + lds[1]) + (lds[2] + lds[3]);
}

__device__ __forceinline__ void better(u64 key, int k, u64 &bkey, int &bk)
{
    if (k >= 0 && (bk < 0 || key > bkey || (key == bkey && k < bk))) bkey = key, bk = k;
}

// atan2(y, x) from rounded +, -, *, / alone (the header states the steps), so that the angle of a component has the same
// bits wherever it is computed - a libm's atan2 is not correctly rounded, and two of them differ in the last place.
// Within 1e-15 relative of the true value.
__device__ __forceinline__ double atan2_series(double y, double x)
{
#pragma clang fp contract(off)
    const double pi = 3.14159265358979323846, ax = fabs(x), ay = fabs(y);
    if (ax == 0.0 && ay == 0.0) return 0.0;
    const bool swap = ay > ax;
    double t = swap ? ax / ay : ay / ax, base = 0.0;  // t in [0, 1]
    if (t > 0.4142135623730950488) {                  // tan(pi / 8): atan t = pi / 4 + atan((t - 1) / (t + 1))
        t = (t - 1.0) / (t + 1.0);
        base = 0.25 * pi;
    }
    const double z = t * t;
    double s = 0.0;
    for (int k = 22; k >= 0; --k) s = 1.0 / (double)(2 * k + 1) - z * s;  // 1 - z / 3 + z^2 / 5 - ... by Horner
    double r = base + t * s;
    if (swap) r = 0.5 * pi - r;
    if (x < 0.0) r = pi - r;
    return y < 0.0 ? 0.0 - r : r;
}

// ---- deblending (the header's DEBLENDING): sub[k], the peak whose basin the cell k of K lies in ---------------------------------
// Six launches in front of src_count_kernel, which then runs on `sub` in place of the labels: a root is a peak.
//     deb_init_kernel     bmax[.] = 0, bidx[.] = INT_MAX
//     deb_max_kernel      bmax[label] = the largest value of the island: 64-bit atomicMax of the bits (all values are > 0)
//     deb_idx_kernel      bidx[label] = the smallest index among the cells that hold it: 32-bit atomicMin
//     deb_up_kernel       up[k] = the highest of k and its 8 neighbours with k's label; the peak counts zeroed
//     deb_summit_kernel   a cell with up[k] == k: the wave scans its window and the cell climbs on, is a peak (counted at
//                         its island), or - a faint summit - hangs below the island's brightest cell
//     deb_chase_kernel    sub[k] = the fixed point of up from k; -1 outside K
// A cell with k's label lies in K as k does (K is whole components of L), so comparing labels is the whole test.
// Only keys are compared and only integers are combined by atomics: sub is a function of the image.
struct DebLayout {
    size_t bmax, bidx, sub, total;
};

DebLayout deb_layout(int64_t N)
{
    DebLayout l;
    const size_t cells = (size_t)N * N;
    l.bmax = 0;  // (u64 per cell; after deb_idx_kernel its first 4 B per cell are the peak counts)
    l.bidx = (cells * 8 + 255) & ~(size_t)255;
    l.sub = l.bidx + ((cells * 4 + 255) & ~(size_t)255);
    l.total = l.sub + ((cells * 4 + 255) & ~(size_t)255);
    return l;
}

__device__ __forceinline__ u64 max_load(const u64 *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__global__ void __launch_bounds__(256) deb_init_kernel(int64_t cells, const AmState *st, u64 *__restrict__ bmax, int *__restrict__ bidx)
{
    if (st->reason != 0) return;
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < cells; k += (int64_t)gridDim.x * 256) {
        bmax[k] = 0;
        bidx[k] = 0x7fffffff;
    }
}

// A wave whose 64 cells all belong to one island reduces by shuffles and sends one lane, as src_box_kernel does; a value
// the slot already holds is not sent (the slot only rises, so a stale read can only cost an atomic, never lose one).
__global__ void __launch_bounds__(256)
    deb_max_kernel(int64_t cells, const AmState *st, const double *__restrict__ image, const int *__restrict__ label,
                   const uint8_t *__restrict__ kbyte, u64 *bmax)
{
    if (st->reason != 0) return;
    const int64_t step = (int64_t)gridDim.x * 256;
    for (int64_t base = (int64_t)blockIdx.x * 256; base < cells; base += step) {  // (uniform over the work-group)
        const int64_t k = base + threadIdx.x;
        int L = -1;
        u64 key = 0;
        if (k < cells && kbyte[k] != 0) L = label[k], key = __builtin_bit_cast(u64, image[k]);
        const int first = __shfl(L, 0);
        if (__all(L == first)) {
            if (first < 0) continue;
            for (int off = 32; off > 0; off >>= 1) {
                const u64 o = __shfl_down(key, off);
                key = o > key ? o : key;
            }
            if ((threadIdx.x & 63) == 0 && key > max_load(bmax + first)) atomicMax(bmax + first, key);
        } else if (L >= 0 && key > max_load(bmax + L)) {
            atomicMax(bmax + L, key);
        }
    }
}

__global__ void __launch_bounds__(256)
    deb_idx_kernel(int64_t cells, const AmState *st, const double *__restrict__ image, const int *__restrict__ label,
                   const uint8_t *__restrict__ kbyte, const u64 *__restrict__ bmax, int *bidx)
{
    if (st->reason != 0) return;
    const int64_t step = (int64_t)gridDim.x * 256;
    for (int64_t base = (int64_t)blockIdx.x * 256; base < cells; base += step) {  // (uniform over the work-group)
        const int64_t k = base + threadIdx.x;
        int L = -1, cand = 0x7fffffff;
        if (k < cells && kbyte[k] != 0) {
            L = label[k];
            if (__builtin_bit_cast(u64, image[k]) == bmax[L]) cand = (int)k;
        }
        const int first = __shfl(L, 0);
        if (__all(L == first)) {
            if (first < 0) continue;
            for (int off = 32; off > 0; off >>= 1) {
                const int o = __shfl_down(cand, off);
                cand = o < cand ? o : cand;
            }
            if ((threadIdx.x & 63) == 0 && cand < box_load(bidx + first)) atomicMin(bidx + first, cand);
        } else if (L >= 0 && cand < box_load(bidx + L)) {
            atomicMin(bidx + L, cand);
        }
    }
}

__global__ void __launch_bounds__(256)
    deb_up_kernel(int64_t N, const AmState *st, const double *__restrict__ image, const int *__restrict__ label,
                  const uint8_t *__restrict__ kbyte, int *__restrict__ up, int *__restrict__ npk)
{
    if (st->reason != 0) return;
    const int64_t cells = N * N;
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < cells; k += (int64_t)gridDim.x * 256) {
        npk[k] = 0;
        if (kbyte[k] == 0) continue;
        const int L = label[k];
        const int64_t y = k / N, x = k - y * N;
        u64 bkey = ordered_bits(image[k]);
        int bk = (int)k;
        for (int64_t ey = (y > 0 ? y - 1 : 0); ey <= (y < N - 1 ? y + 1 : N - 1); ++ey)
            for (int64_t ex = (x > 0 ? x - 1 : 0); ex <= (x < N - 1 ? x + 1 : N - 1); ++ex) {
                const int64_t e = ey * N + ex;
                if (label[e] == L) better(ordered_bits(image[e]), (int)e, bkey, bk);
            }
        up[k] = bk;
    }
}

// The summits of a wave's 64 cells are taken one after the other; the wave's lanes share the window's cells.
__global__ void __launch_bounds__(256)
    deb_summit_kernel(int64_t N, int r, const AmState *st, const double *__restrict__ image, const int *__restrict__ label,
                      const uint8_t *__restrict__ kbyte, const int *__restrict__ bidx, int *up, int *npk)
{
    if (st->reason != 0) return;
    const int64_t cells = N * N, step = (int64_t)gridDim.x * 256;
    const int lane = threadIdx.x & 63;
    const double T_hi = st->T_hi;
    for (int64_t base = (int64_t)blockIdx.x * 256; base < cells; base += step) {  // (uniform over the work-group)
        const int64_t k = base + threadIdx.x;
        u64 todo = __ballot(k < cells && kbyte[k] != 0 && up[k] == (int)k);  // (up[k] is written by k's own lane alone)
        while (todo) {
            const int src = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const int ks = __shfl((int)k, src), L = label[ks];
            const int ys = (int)(ks / N), xs = (int)(ks - (int64_t)ys * N);
            const int y0 = ys - r > 0 ? ys - r : 0, y1 = ys + r < N - 1 ? ys + r : (int)N - 1;
            const int x0 = xs - r > 0 ? xs - r : 0, x1 = xs + r < N - 1 ? xs + r : (int)N - 1;
            const int w = x1 - x0 + 1, n = w * (y1 - y0 + 1);  // at most 65 x 65
            u64 bkey = 0;
            int bk = -1;
            for (int i = lane; i < n; i += 64) {
                const int64_t e = (int64_t)(y0 + i / w) * N + x0 + i % w;
                if (label[e] == L) better(ordered_bits(image[e]), (int)e, bkey, bk);
            }
            for (int o = 32; o > 0; o >>= 1) {
                const u64 okey = __shfl_down(bkey, o);
                const int ok = __shfl_down(bk, o);
                better(okey, ok, bkey, bk);
            }
            bk = __shfl(bk, 0);  // W(ks): never -1, the window holds ks
            if (lane == src) {
                if (bk >= 0 && bk != ks)
                    up[ks] = bk;
                else if (image[ks] > T_hi)
                    atomicAdd(npk + L, 1);
                else
                    up[ks] = bidx[L];
            }
        }
    }
}

// An ascent ends because every step goes to a strictly higher cell.  The fixed point found is stored over up[k] as well, so
// that an ascent that starts later through k is shorter: a reader finds the old pointer or the new one, both lead to the same
// fixed point, and a fixed point's own pointer is never written.  These loads are relaxed agent-scope atomics for that.
__global__ void __launch_bounds__(256)
    deb_chase_kernel(int64_t cells, const AmState *st, const uint8_t *__restrict__ kbyte, int *up, int *__restrict__ sub)
{
    if (st->reason != 0) return;
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < cells; k += (int64_t)gridDim.x * 256) {
        if (kbyte[k] == 0) {
            sub[k] = -1;
            continue;
        }
        int x = (int)k;
        int hops = 0;
        for (;; ++hops) {
            const int p = box_load(up + x);
            if (p == x || p < 0 || p >= cells) break;  // (p outside the image cannot be: it would end the loop, never extend it)
            x = p;
        }
        if (hops > 1) __hip_atomic_store(up + k, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        sub[k] = x;
    }
}

// One work-group per row (a work-group strides over the rows when there are more rows than work-groups).  With deblending
// `label` is sub, a root is a peak, island[root] is its island's label and npk[that] the island's peaks; else both are NULL.
__global__ void __launch_bounds__(256)
    src_measure_kernel(int64_t N, double theta, int64_t border, const AmState *st, const double *__restrict__ image,
                       const int *__restrict__ label, const int *__restrict__ roots, const int *__restrict__ boxes,
                       const int64_t *__restrict__ count, int64_t max_c, const double *__restrict__ beam, int correct,
                       const int *__restrict__ island, const int *__restrict__ npk, double *__restrict__ comps,
                       double *__restrict__ info)
{
#pragma clang fp contract(off)
    __shared__ u64 pk_key[4];
    __shared__ int pk_idx[4];
    __shared__ double lds[4];
    if (st->reason != 0) return;
    const int64_t found = *count, nrows = found < max_c ? found : max_c;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t row = blockIdx.x; row < nrows; row += gridDim.x) {
        const int root = roots[row];
        const int y0 = boxes[4 * row + 0], y1 = boxes[4 * row + 1], x0 = boxes[4 * row + 2], x1 = boxes[4 * row + 3];
        // cell i = t, t + 256, ... of the box in row-major order is (by, bx), kept without a division per cell
        const int w = x1 - x0 + 1, h = y1 - y0 + 1, qw = 256 / w, rw = 256 % w;
        const int by0 = (int)threadIdx.x / w, bx0 = (int)threadIdx.x % w;
        // walk 1: the peak
        u64 bkey = 0;
        int bk = -1;
        for (int by = by0, bx = bx0; by < h;) {
            const int64_t k = (int64_t)(y0 + by) * N + x0 + bx;
            if (label[k] == root) better(ordered_bits(image[k]), (int)k, bkey, bk);
            bx += rw, by += qw;
            if (bx >= w) bx -= w, by += 1;
        }
        for (int o = 32; o > 0; o >>= 1) {
            const u64 okey = __shfl_down(bkey, o);
            const int ok = __shfl_down(bk, o);
            better(okey, ok, bkey, bk);
        }
        __syncthreads();  // (the last row's peak has been read)
        if (lane == 0) pk_key[wave] = bkey, pk_idx[wave] = bk;
        __syncthreads();
        bkey = pk_key[0], bk = pk_idx[0];
        for (int wv = 1; wv < 4; ++wv) better(pk_key[wv], pk_idx[wv], bkey, bk);
        if (bk < 0) continue;  // (cannot be: the root lies in the box.  Uniform over the work-group)
        const int yp = (int)(bk / N), xp = (int)(bk - (int64_t)yp * N);
        // walk 2: the count and the sums about (yp, xp)
        double n = 0.0, S = 0.0, Sx = 0.0, Sy = 0.0, Sxx = 0.0, Sxy = 0.0, Syy = 0.0;
        for (int by = by0, bx = bx0; by < h;) {
            const int64_t k = (int64_t)(y0 + by) * N + x0 + bx;
            if (label[k] == root) {
                const double v = image[k];
                const int64_t dx = x0 + bx - xp, dy = y0 + by - yp;
                n += 1.0;
                S += v;
                Sx += v * (double)dx;
                Sy += v * (double)dy;
                Sxx += v * (double)(dx * dx);
                Sxy += v * (double)(dx * dy);
                Syy += v * (double)(dy * dy);
            }
            bx += rw, by += qw;
            if (bx >= w) bx -= w, by += 1;
        }
        n = tree_sum256(n, lds);
        S = tree_sum256(S, lds);
        Sx = tree_sum256(Sx, lds);
        Sy = tree_sum256(Sy, lds);
        Sxx = tree_sum256(Sxx, lds);
        Sxy = tree_sum256(Sxy, lds);
        Syy = tree_sum256(Syy, lds);
        if (threadIdx.x != 0) continue;
        const double nan = __builtin_nan(""), pi = 3.14159265358979323846, Pi = image[bk];
        // 1  centroid and covariance
        const double ox = Sx / S, oy = Sy / S;
        const double cx = (double)xp + ox, cy = (double)yp + oy;
        double mxx = Sxx / S - ox * ox, mxy = Sxy / S - ox * oy, myy = Syy / S - oy * oy;
        double F = S;
        // 2  the truncation at the isophote T_lo
        if (correct) {
            const double t = st->T_lo / Pi;
            if (t > 0.0) {
                const double u = 1.0 - t, g = u / (1.0 - t * (1.0 - log(t)));
                F = F / u;
                mxx = mxx * g, mxy = mxy * g, myy = myy * g;
            }
        }
        // 3  the beam
        int flags = 0;
        double ixx = mxx, ixy = mxy, iyy = myy;
        bool shaped = true;
        if (beam) {
            const double A = beam[0], B = beam[1], C = beam[2];
            if (beam_usable(A, B, C, beam[7])) {
                const double det = A * C - B * B, two = 2.0 * det;
                F = F * sqrt(det) / pi;
                ixx = mxx - C / two, ixy = mxy + B / two, iyy = myy - A / two;
            } else {
                flags |= 4;
                shaped = false;
            }
        }
        // 4  the shape
        double bmaj = 0.0, bmin = 0.0, bpa = 0.0;
        if (!shaped) {
            F = bmaj = bmin = bpa = nan;
        } else {
            const double d2 = ixx * iyy - ixy * ixy;
            if (ixx > 0.0 && iyy > 0.0 && d2 > 0.0) {
                const double h = 0.5 * (ixx + iyy), d = 0.5 * (ixx - iyy), q = sqrt(d * d + ixy * ixy);
                const double lp = h + q, lm = d2 / lp, c = 8.0 * 0.693147180559945309417;
                bmaj = sqrt(c * lp) * theta / (double)N;
                bmin = sqrt(c * lm) * theta / (double)N;
                bpa = 0.5 * pi - 0.5 * atan2_series(2.0 * ixy, ixx - iyy);
                if (bpa > 0.5 * pi) bpa -= pi;
            } else {
                flags |= 1;
            }
        }
        if (y0 <= border || x0 <= border || y1 >= N - 1 - border || x1 >= N - 1 - border) flags |= 2;
        const int isl = island ? island[root] : root;
        if (npk && npk[isl] > 1) flags |= 8;
        // 5  the position
        const double half = (double)(N / 2);
        double *o = comps + row * GRIDHIP_COMP_DOUBLES;
        o[0] = theta * (cx - half) / (double)N;
        o[1] = theta * (cy - half) / (double)N;
        o[2] = F;
        o[3] = 0.0, o[4] = 0.0, o[5] = 0.0;
        o[6] = bmaj, o[7] = bmin, o[8] = bpa;
        o[9] = 0.0;
        if (info) {
            double *q = info + row * SRC_INFO;
            q[0] = (double)isl, q[1] = n, q[2] = (double)yp, q[3] = (double)xp, q[4] = Pi;
            q[5] = S, q[6] = Sx, q[7] = Sy, q[8] = Sxx, q[9] = Sxy, q[10] = Syy;
            q[11] = (double)y0, q[12] = (double)y1, q[13] = (double)x0, q[14] = (double)x1;
            q[15] = (double)flags;
        }
    }
}

__global__ void src_stats_kernel(const AmState *st, const int64_t *__restrict__ count, int64_t max_c,
                                 const double *__restrict__ comps, double *__restrict__ stats)
{
    if (st->reason != 0) return;  // (am_levels_kernel wrote them, and the scan a count of 0)
    const int64_t found = *count, nrows = found < max_c ? found : max_c;
    double flux = 0.0, points = 0.0;
    for (int64_t r = 0; r < nrows; ++r) {
        const double *c = comps + r * GRIDHIP_COMP_DOUBLES;
        flux += c[2];
        if (c[6] == 0.0 && c[7] == 0.0) points += 1.0;
    }
    stats[0] = st->T_hi;
    stats[1] = st->T_lo;
    stats[2] = st->P;
    stats[3] = (double)found;
    stats[4] = (double)nrows;
    stats[5] = points;
    stats[6] = flux;
    stats[7] = 0.0;
}

}  // namespace

int sources_check(gridhip_ctx *ctx, double theta, int64_t lam, const double *image, int64_t border, double thr_hi,
                  double thr_lo, double nsigma_hi, double nsigma_lo, const double *noise, double peak_frac,
                  int64_t min_cells, const double *beam, int correct, int64_t max_c, const double *comps, const double *info,
                  const int64_t *count, const double *stats, int64_t *N)
{
    *N = gridhip_image_size(theta, lam);
    if (ctx->img->sources_deblend > SRC_MAX_DEBLEND)
        return fail(ctx, GRIDHIP_EINVAL, "find_sources: option 'sources_deblend' above %d", (int)SRC_MAX_DEBLEND);
    if (!count || !stats || max_c < 0 || (max_c > 0 && !comps) || (correct != 0 && correct != 1))
        return fail(ctx, GRIDHIP_EINVAL, "find_sources: max_c >= 0, comps, count, stats, correct in {0, 1}");
    GH_CHECK(automask_levels_check(ctx, "find_sources", *N, image, border, thr_hi, thr_lo, nsigma_hi, nsigma_lo, noise,
                                   peak_frac, min_cells));
    if (*N <= SRC_MAX_N) {  // (above it the call is refused below, and the byte counts are not needed)
        const size_t cb = (size_t)max_c * GRIDHIP_COMP_DOUBLES * 8, ib = (size_t)max_c * SRC_INFO * 8;
        if (outputs_clash({{comps, cb}, {info, ib}, {count, 8}, {stats, 64}},
                          {{image, (size_t)*N * *N * 8}, {beam, 64}, {noise, 8}}))
            return fail(ctx, GRIDHIP_EINVAL, "find_sources: comps, info, count and stats may overlap nothing");
    }
    if (*N > SRC_MAX_N) return fail(ctx, GRIDHIP_EUNSUPPORTED, "find_sources: N above %d", (int)SRC_MAX_N);
    return GRIDHIP_OK;
}

size_t sources_scratch_bytes(int64_t N, int64_t max_c) { return layout(N, max_c).total; }

int sources_run(gridhip_ctx *ctx, int64_t N, double theta, const double *image, int64_t border, double thr_hi,
                double thr_lo, double nsigma_hi, double nsigma_lo, const double *noise, double peak_frac, int64_t min_cells,
                const double *beam, int correct, int64_t max_c, double *comps, double *info, int64_t *count, double *stats,
                void *am_scratch, void *scratch)
{
    GH_CHECK(automask_label_run(ctx, N, image, border, 0, thr_hi, thr_lo, nsigma_hi, nsigma_lo, noise, peak_frac, min_cells,
                                stats, am_scratch));
    const AmPlanes p = automask_planes(ctx, N, am_scratch);
    const SrcLayout l = layout(N, max_c);
    char *base = reinterpret_cast<char *>(scratch);
    unsigned int *segcount = reinterpret_cast<unsigned int *>(base + l.segcount);
    int64_t *offs = reinterpret_cast<int64_t *>(base + l.offs);
    int *roots = reinterpret_cast<int *>(base + l.roots), *boxes = reinterpret_cast<int *>(base + l.boxes);
    const int64_t cells = N * N;
    const AmState *st = p.state;
    const dim3 seggrid = grid_for(ctx, l.nseg, 1), flat = grid_for(ctx, cells);
    const uint8_t *kbyte = p.kbyte;
    hipStream_t s = ctx->stream;
    // what the kernels below take for labels: the islands', or with deblending the basins'
    const int *lab = p.label, *island = nullptr, *npk = nullptr;
    DevBuf deb;  // (handed back to the pool at the return: what is enqueued later on this stream runs after these kernels)
    const int r = (int)ctx->img->sources_deblend;
    if (r > 0) {
        const DebLayout d = deb_layout(N);
        GH_CHECK(deb.alloc(ctx, d.total));
        char *db = deb.as<char>();
        u64 *bmax = reinterpret_cast<u64 *>(db + d.bmax);
        int *bidx = reinterpret_cast<int *>(db + d.bidx), *sub = reinterpret_cast<int *>(db + d.sub);
        int *peaks = reinterpret_cast<int *>(bmax), *up = p.spare;
        hipLaunchKernelGGL(deb_init_kernel, flat, dim3(256), 0, s, cells, st, bmax, bidx);
        hipLaunchKernelGGL(deb_max_kernel, flat, dim3(256), 0, s, cells, st, image, lab, kbyte, bmax);
        hipLaunchKernelGGL(deb_idx_kernel, flat, dim3(256), 0, s, cells, st, image, lab, kbyte, (const u64 *)bmax, bidx);
        hipLaunchKernelGGL(deb_up_kernel, flat, dim3(256), 0, s, N, st, image, lab, kbyte, up, peaks);
        hipLaunchKernelGGL(deb_summit_kernel, flat, dim3(256), 0, s, N, r, st, image, lab, kbyte, (const int *)bidx, up, peaks);
        hipLaunchKernelGGL(deb_chase_kernel, flat, dim3(256), 0, s, cells, st, kbyte, up, sub);
        island = lab, npk = peaks, lab = sub;
    }
    hipLaunchKernelGGL(src_count_kernel, seggrid, dim3(256), 0, s, cells, st, lab, kbyte, l.nseg, segcount);
    GH_CHECK(segment_scan(ctx, l.nseg, segcount, offs, count));
    if (max_c > 0) {
        hipLaunchKernelGGL(src_scatter_kernel, seggrid, dim3(256), 0, s, N, st, lab, kbyte, l.nseg, (const int64_t *)offs, max_c,
                           p.spare, roots, boxes);
        hipLaunchKernelGGL(src_box_kernel, flat, dim3(256), 0, s, N, st, lab, kbyte, (const int *)p.spare, max_c, boxes);
        hipLaunchKernelGGL(src_measure_kernel, grid_for(ctx, max_c, 1), dim3(256), 0, s, N, theta, border, st, image, lab,
                           (const int *)roots, (const int *)boxes, (const int64_t *)count, max_c, beam, correct, island, npk,
                           comps, info);
    }
    hipLaunchKernelGGL(src_stats_kernel, dim3(1), dim3(1), 0, s, st, (const int64_t *)count, max_c, (const double *)comps,
                       stats);
    GH_CHECK_HIP(ctx, hipGetLastError());
    return GRIDHIP_OK;
}

}  // namespace gridhip

using namespace gridhip;

namespace {

int find_sources_any(gridhip_ctx *ctx, bool dev, double theta, int64_t lam, const double *image, int64_t border,
                     double thr_hi, double thr_lo, double nsigma_hi, double nsigma_lo, const double *noise, double peak_frac,
                     int64_t min_cells, const double *beam, int correct, int64_t max_c, double *comps, double *info,
                     int64_t *count, double *stats)
{
    if (!ctx) return GRIDHIP_EINVAL;
    int64_t N = 0;
    GH_CHECK(sources_check(ctx, theta, lam, image, border, thr_hi, thr_lo, nsigma_hi, nsigma_lo, noise, peak_frac, min_cells,
                           beam, correct, max_c, comps, info, count, stats, &N));
    if (!dev && beam && !beam_usable(beam[0], beam[1], beam[2], beam[7]))
        return fail(ctx, GRIDHIP_EINVAL, "find_sources: the beam's fit failed, or A, B, C are not finite and positive definite");
    GH_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    DevBuf am, scratch;
    GH_CHECK(am.alloc(ctx, automask_scratch_bytes(ctx, N)));
    GH_CHECK(scratch.alloc(ctx, sources_scratch_bytes(N, max_c)));
    Staged st(ctx, dev);
    image = st.in(image, (size_t)N * N * 8), noise = st.in(noise, 8), beam = st.in(beam, 64);
    double *dc = st.raw(comps, (size_t)max_c * GRIDHIP_COMP_DOUBLES * 8), *di = st.raw(info, (size_t)max_c * SRC_INFO * 8);
    int64_t *dn = st.raw(count, 8);
    double *ds = st.out(stats, 64);
    GH_CHECK(st.status());
    GH_CHECK(sources_run(ctx, N, theta, image, border, thr_hi, thr_lo, nsigma_hi, nsigma_lo, noise, peak_frac, min_cells, beam,
                         correct, max_c, dc, di, dn, ds, am.p, scratch.p));
    if (dev) return GRIDHIP_OK;
    // only the rows written come back: the caller's rows after them stay as they were
    int64_t found = 0;
    GH_CHECK(d2h(ctx, &found, dn, 8));
    GH_CHECK(sync(ctx));
    const size_t rows = (size_t)(found < max_c ? found : max_c);
    GH_CHECK(d2h(ctx, comps, dc, rows * GRIDHIP_COMP_DOUBLES * 8));
    if (info) GH_CHECK(d2h(ctx, info, di, rows * SRC_INFO * 8));
    GH_CHECK(st.finish());
    *count = found;
    return GRIDHIP_OK;
}

}  // namespace

extern "C" {

int gridhip_find_sources(gridhip_ctx *ctx, double theta, int64_t lam, const double *image, int64_t border, double thr_hi,
                         double thr_lo, double nsigma_hi, double nsigma_lo, const double *noise, double peak_frac,
                         int64_t min_cells, const double *beam, int correct, int64_t max_c, double *comps, double *info,
                         int64_t *count, double *stats)
{
    return find_sources_any(ctx, false, theta, lam, image, border, thr_hi, thr_lo, nsigma_hi, nsigma_lo, noise, peak_frac,
                            min_cells, beam, correct, max_c, comps, info, count, stats);
}

int gridhip_find_sources_dev(gridhip_ctx *ctx, double theta, int64_t lam, const double *image, int64_t border, double thr_hi,
                             double thr_lo, double nsigma_hi, double nsigma_lo, const double *noise, double peak_frac,
                             int64_t min_cells, const double *beam, int correct, int64_t max_c, double *comps, double *info,
                             int64_t *count, double *stats)
{
    return find_sources_any(ctx, true, theta, lam, image, border, thr_hi, thr_lo, nsigma_hi, nsigma_lo, noise, peak_frac,
                            min_cells, beam, correct, max_c, comps, info, count, stats);
}

}  // extern "C"
