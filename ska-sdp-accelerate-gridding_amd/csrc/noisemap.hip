// Local background and noise maps (include/gridhip.h, "local background and noise maps"): the lower median and the MAD of
// a (2 half + 1)^2 window around every node of a mesh, sigma-clipped, and the two tables interpolated onto the image.
//
// One call is three launches whatever the image holds:
//     nm_node_kernel    one work-group per node.  The window's cells go into LDS as image_stats' 64-bit keys - a cell that
//                       does not take part as NM_DEAD, the key of no finite double - and every select of every clip round
//                       runs out of that one copy: a most-significant-digit radix select with 8-bit digits for the median,
//                       the same over the keys of d = |v - median| recomputed from the stored keys for the MAD, then a pass
//                       that overwrites the cells with d > L by NM_DEAD.  No second buffer: at half = 64 the keys are
//                       129 x 129 x 8 = 133,128 B of the 160 KB a work-group may take.
//     nm_map_kernel     one pass over the image: the bilinear interpolation of the background and rms tables, written to
//                       the maps, and image - background or (image - background) / rms to out
//     nm_stats_kernel   one work-group: the 8 stats from the node table and the map kernel's count
// The histogram of a pass is 256 32-bit LDS counters, and every lane adds to them singly.  In a noise window nearly all keys
// share their high digits, so the first passes of a select add to a handful of addresses; three ways round that were built
// and measured - the context option "noisemap_hist" still selects them (bit 0: skip the prefix that the window's smallest
// and largest key share; bit 1: one histogram copy per wave; bit 2: lanes of a wave with the same digit add once, for up to
// four digits per step, the rest add singly) - and each of them was slower than the plain histogram on gfx950, by 8 to 90 %:
// DESIGN.md section 9 has the numbers.
// Counts are integers, keys are compared as integers, and d, L and the interpolation are fixed sequences of rounded
// operations under fp contract(off): there is no floating-point atomic and no sum of doubles, and the result is the same
// bits on every run.
#include "common.h"
#include "imaging.h"

namespace gridhip {

namespace {

typedef unsigned long long u64;

constexpr u64 EXP_MASK = 0x7ff0000000000000ULL;
constexpr u64 NM_DEAD = ~(u64)0;  // (ordered_value gives a NaN: no cell that takes part has this key)
constexpr int64_t NM_MAX_HALF = 64;
constexpr int NM_MAX_WAVES = 16;
constexpr int NM_MAP_ROWS = 16;  // rows of one work-group of the map kernel: CLEAN_MAX_N / 16 rows of work-groups fit a grid

struct NmMesh {
    int64_t N, border, step, M, G;
};

__host__ __device__ inline int64_t nm_centre(const NmMesh &m, int64_t i)
{
    int64_t t = i * m.step + m.step / 2;
    if (t > m.M - 1) t = m.M - 1;
    return m.border + t;
}

__device__ __forceinline__ bool nm_finite(double v) { return (__builtin_bit_cast(u64, v) & EXP_MASK) != EXP_MASK; }

struct NmShared {
    u64 red[2][NM_MAX_WAVES];
    unsigned int cnt, digit, rank, pad;
};

// the sum of x over the work-group (every thread gets it)
__device__ __forceinline__ unsigned int nm_block_sum(unsigned int x, NmShared &sh)
{
    if (threadIdx.x == 0) sh.cnt = 0;
    __syncthreads();
    for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o);
    if ((threadIdx.x & 63) == 0 && x) atomicAdd(&sh.cnt, x);
    __syncthreads();
    const unsigned int r = sh.cnt;
    __syncthreads();
    return r;
}

// the key a select orders a live cell by: MODE 0 its own, MODE 1 that of |v - med|, the difference rounded once
template <int MODE>
__device__ __forceinline__ u64 nm_key(u64 k, double med)
{
#pragma clang fp contract(off)
    return MODE == 0 ? k : ordered_bits(fabs(ordered_value(k) - med));
}

// The key of rank `rank` among the live cells of keys[0, cells), by a radix select from the top digit down.  Every thread
// of the work-group calls it with the same arguments and gets the same key; rank is below the number of live cells.
// bins: ncopy x 256 counters.
template <int MODE>
__device__ u64 nm_select(const u64 *keys, int cells, unsigned int rank, double med, unsigned int *bins, int strat,
                         NmShared &sh)
{
    const int t = threadIdx.x, T = blockDim.x, lane = t & 63, wave = t >> 6, nw = T >> 6;
    const int ncopy = (strat & 2) ? nw : 1;
    u64 prefix = 0;
    int top = 64;  // the bits below `top` are still to be chosen
    if (strat & 1) {
        u64 lo = ~(u64)0, hi = 0;
        for (int i = t; i < cells; i += T) {
            const u64 k = keys[i];
            if (k != NM_DEAD) {
                const u64 q = nm_key<MODE>(k, med);
                lo = q < lo ? q : lo;
                hi = q > hi ? q : hi;
            }
        }
        for (int o = 32; o > 0; o >>= 1) {
            const u64 a = __shfl_down(lo, o), b = __shfl_down(hi, o);
            lo = a < lo ? a : lo;
            hi = b > hi ? b : hi;
        }
        if (lane == 0) sh.red[0][wave] = lo, sh.red[1][wave] = hi;
        __syncthreads();
        lo = sh.red[0][0], hi = sh.red[1][0];
        for (int w = 1; w < nw; ++w) {
            lo = sh.red[0][w] < lo ? sh.red[0][w] : lo;
            hi = sh.red[1][w] > hi ? sh.red[1][w] : hi;
        }
        __syncthreads();
        if (lo == hi) return lo;
        top = 64 - __clzll((long long)(lo ^ hi));
        prefix = top == 64 ? 0 : (hi >> top) << top;
    }
    const int iters = (cells + T - 1) / T;
    unsigned int *mine = bins + ((strat & 2) ? wave * 256 : 0);
    while (top > 0) {
        const int shift = top > 8 ? top - 8 : 0, nb = 1 << (top - shift);
        for (int i = t; i < ncopy * 256; i += T) bins[i] = 0;
        __syncthreads();
        for (int it = 0; it < iters; ++it) {  // (the same trip count for every lane: the ballots below need whole waves)
            const int i = it * T + t;
            bool take = false;
            unsigned int d = 0;
            if (i < cells) {
                const u64 k = keys[i];
                if (k != NM_DEAD) {
                    const u64 q = nm_key<MODE>(k, med);
                    if (top == 64 || ((q ^ prefix) >> top) == 0) {
                        take = true;
                        d = (unsigned int)(q >> shift) & (unsigned int)(nb - 1);
                    }
                }
            }
            if (strat & 4) {
                u64 m = __ballot(take);
                for (int a = 0; a < 4 && m; ++a) {
                    const int leader = __ffsll((long long)m) - 1;
                    const unsigned int d0 = __shfl(d, leader);
                    const u64 same = __ballot(take && d == d0);
                    if (lane == leader) atomicAdd(&mine[d0], (unsigned int)__popcll(same));
                    if (d == d0) take = false;
                    m &= ~same;
                }
            }
            if (take) atomicAdd(&mine[d], 1u);
        }
        __syncthreads();
        if (wave == 0) {  // lane l owns the bins 4 l .. 4 l + 3 of the sum of the copies
            unsigned int c[4], s = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int b = lane * 4 + j;
                c[j] = 0;
                if (b < nb)
                    for (int w = 0; w < ncopy; ++w) c[j] += bins[w * 256 + b];
                s += c[j];
            }
            unsigned int inc = s;
            for (int o = 1; o < 64; o <<= 1) {
                const unsigned int u = __shfl_up(inc, o);
                if (lane >= o) inc += u;
            }
            const unsigned int exc = inc - s;
            if (s > 0 && rank >= exc && rank < inc) {  // (exactly one lane)
                unsigned int below = exc;
                int dsel = -1;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (dsel < 0 && rank < below + c[j]) dsel = lane * 4 + j;
                    if (dsel < 0) below += c[j];
                }
                sh.digit = (unsigned int)dsel;
                sh.rank = rank - below;
            }
        }
        __syncthreads();
        prefix |= (u64)sh.digit << shift;
        rank = sh.rank;
        top = shift;
        // (sh.digit is written again only after the next pass's two barriers; the bins are zeroed after this one)
    }
    return prefix;
}

// dynamic LDS: (2 half + 1)^2 keys, then ncopy x 256 counters
__global__ void __launch_bounds__(1024)
    nm_node_kernel(NmMesh m, int64_t half, const double *__restrict__ image, const uint8_t *__restrict__ mask, int exclude,
                   double kappa, int nclip, int64_t min_count, int strat, double *__restrict__ nodes, u64 *counter)
{
#pragma clang fp contract(off)
    extern __shared__ u64 nm_lds[];
    __shared__ NmShared sh;
    const int t = threadIdx.x, T = blockDim.x;
    const int side = 2 * (int)half + 1;
    u64 *keys = nm_lds;
    unsigned int *bins = reinterpret_cast<unsigned int *>(nm_lds + (size_t)side * side);
    if (blockIdx.x == 0 && t == 0) *counter = 0;  // (the map kernel's count of cells; it runs after this kernel)
    const int64_t G2 = m.G * m.G, last = m.N - m.border - 1;
    const double nan = __builtin_nan("");
    for (int64_t node = blockIdx.x; node < G2; node += gridDim.x) {
        const int64_t cy = nm_centre(m, node / m.G), cx = nm_centre(m, node % m.G);
        const int64_t y0 = cy - half < m.border ? m.border : cy - half, y1 = cy + half > last ? last : cy + half;
        const int64_t x0 = cx - half < m.border ? m.border : cx - half, x1 = cx + half > last ? last : cx + half;
        const int w = (int)(x1 - x0 + 1), cells = w * (int)(y1 - y0 + 1);  // (at most side * side)
        unsigned int live = 0;
        for (int i = t; i < cells; i += T) {
            const int64_t k = (y0 + i / w) * m.N + x0 + i % w;
            const double v = image[k];
            const bool ok = nm_finite(v) && (!mask || (mask[k] != 0) != (exclude != 0));
            keys[i] = ok ? ordered_bits(v) : NM_DEAD;
            live += ok ? 1u : 0u;
        }
        unsigned int n = nm_block_sum(live, sh);  // (its barriers also publish the keys)
        int r = 0;
        double med = nan, mad = nan;
        while (n > 0) {
            med = ordered_value(nm_select<0>(keys, cells, (n - 1) / 2, 0.0, bins, strat, sh));
            mad = ordered_value(nm_select<1>(keys, cells, (n - 1) / 2, med, bins, strat, sh));
            if (r == nclip) break;
            const double sigma = 1.4826 * mad;
            const double L = kappa * sigma;
            unsigned int dropped = 0;
            for (int i = t; i < cells; i += T) {
                const u64 k = keys[i];
                if (k != NM_DEAD && fabs(ordered_value(k) - med) > L) {
                    keys[i] = NM_DEAD;
                    dropped += 1;
                }
            }
            dropped = nm_block_sum(dropped, sh);
            if (dropped == 0) break;
            n -= dropped;
            r += 1;
        }
        if (t == 0) {
            const bool enough = (int64_t)n >= min_count;
            nodes[node] = enough ? med : nan;
            nodes[G2 + node] = enough && mad > 0.0 ? 1.4826 * mad : nan;
            nodes[2 * G2 + node] = (double)n;
            nodes[3 * G2 + node] = (double)r;
        }
        __syncthreads();  // (the next node overwrites the keys)
    }
}

// the nodes either side of coordinate p inside the border region, and the weight of the second
__device__ __forceinline__ void nm_locate(const NmMesh &m, int64_t p, int64_t *i, int64_t *i1, double *f)
{
    const int64_t q = p - m.border, h = m.step / 2;
    // the largest i with c_i <= p: the clamp of c_i to M - 1 acts for M < step only, where G is 1
    int64_t a = q < h ? 0 : (q - h) / m.step;
    if (a > m.G - 1) a = m.G - 1;
    const int64_t b = a + 1 < m.G ? a + 1 : m.G - 1;
    const int64_t ca = nm_centre(m, a), cb = nm_centre(m, b);
    *i = a, *i1 = b;
    *f = (b == a || p < ca) ? 0.0 : (double)(p - ca) / (double)(cb - ca);
}

__device__ __forceinline__ double nm_lerp(double a, double b, double f)
{
#pragma clang fp contract(off)
    const bool fa = nm_finite(a), fb = nm_finite(b);
    if (fa && fb) {
        const double d = b - a;
        const double p = f * d;
        return a + p;
    }
    return fa ? a : fb ? b : __builtin_nan("");
}

__device__ __forceinline__ double nm_bilinear(const double *__restrict__ tab, int64_t G, int64_t i, int64_t i1, int64_t j,
                                              int64_t j1, double fy, double fx)
{
    const double top = nm_lerp(tab[i * G + j], tab[i * G + j1], fx);
    const double bot = nm_lerp(tab[i1 * G + j], tab[i1 * G + j1], fx);
    return nm_lerp(top, bot, fy);
}

// A work-group is 256 columns by NM_MAP_ROWS rows; a thread keeps its column and its column's two nodes, the rows' are in
// LDS.  out may be image: a thread reads its cell before it writes it.
__global__ void __launch_bounds__(256)
    nm_map_kernel(NmMesh m, const double *image, const double *__restrict__ nodes, int mode, double *__restrict__ background,
                  double *__restrict__ rms, double *out, u64 *counter)
{
#pragma clang fp contract(off)
    if (!background && !rms && mode == 0) return;  // (the launch count is fixed; a call for the node table alone ends here)
    __shared__ int64_t row_i[NM_MAP_ROWS], row_i1[NM_MAP_ROWS];
    __shared__ double row_f[NM_MAP_ROWS];
    const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x, yb = (int64_t)blockIdx.y * NM_MAP_ROWS;
    const int64_t G2 = m.G * m.G;
    if (threadIdx.x < NM_MAP_ROWS) {  // the rows' nodes once per work-group: no division per cell
        const int64_t y = yb + threadIdx.x;
        int64_t i = 0, i1 = 0;
        double fy = 0.0;
        if (y >= m.border && y < m.N - m.border) nm_locate(m, y, &i, &i1, &fy);
        row_i[threadIdx.x] = i, row_i1[threadIdx.x] = i1, row_f[threadIdx.x] = fy;
    }
    __syncthreads();
    const bool xin = x >= m.border && x < m.N - m.border;
    const double nan = __builtin_nan("");
    int64_t j = 0, j1 = 0;
    double fx = 0.0;
    if (xin) nm_locate(m, x, &j, &j1, &fx);
    unsigned int bad = 0;
    if (x < m.N) {
        for (int r = 0; r < NM_MAP_ROWS; ++r) {
            const int64_t y = yb + r;
            if (y >= m.N) break;
            const int64_t k = y * m.N + x;
            double bg = nan, sg = nan, o = nan;
            if (xin && y >= m.border && y < m.N - m.border) {
                const int64_t i = row_i[r], i1 = row_i1[r];
                const double fy = row_f[r];
                bg = nm_bilinear(nodes, m.G, i, i1, j, j1, fy, fx);
                if (rms || mode == 2) sg = nm_bilinear(nodes + G2, m.G, i, i1, j, j1, fy, fx);
                if (mode != 0) {
                    const double diff = image[k] - bg;
                    o = mode == 1 ? diff : diff / sg;
                    bad += nm_finite(o) ? 0u : 1u;
                }
            }
            if (background) background[k] = bg;
            if (rms) rms[k] = sg;
            if (mode != 0) out[k] = o;
        }
    }
    for (int o = 32; o > 0; o >>= 1) bad += __shfl_down(bad, o);
    if ((threadIdx.x & 63) == 0 && bad) atomicAdd(counter, (u64)bad);
}

// one work-group of 256 threads
__global__ void __launch_bounds__(256) nm_stats_kernel(NmMesh m, const double *__restrict__ nodes, int mode, const u64 *counter,
                                                       double *stats)
{
    __shared__ u64 red[5][4];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int64_t G2 = m.G * m.G;
    u64 nbg = 0, nrms = 0, kmin = ~(u64)0, kmax = 0, rounds = 0;
    for (int64_t i = t; i < G2; i += 256) {
        const double bg = nodes[i], sg = nodes[G2 + i];
        nbg += bg == bg ? 1 : 0;
        if (sg == sg) {
            const u64 k = ordered_bits(sg);
            nrms += 1;
            kmin = k < kmin ? k : kmin;
            kmax = k > kmax ? k : kmax;
        }
        const u64 r = (u64)nodes[3 * G2 + i];
        rounds = r > rounds ? r : rounds;
    }
    for (int o = 32; o > 0; o >>= 1) {
        nbg += __shfl_down(nbg, o);
        nrms += __shfl_down(nrms, o);
        const u64 a = __shfl_down(kmin, o), b = __shfl_down(kmax, o), c = __shfl_down(rounds, o);
        kmin = a < kmin ? a : kmin;
        kmax = b > kmax ? b : kmax;
        rounds = c > rounds ? c : rounds;
    }
    if (lane == 0) red[0][wave] = nbg, red[1][wave] = nrms, red[2][wave] = kmin, red[3][wave] = kmax, red[4][wave] = rounds;
    __syncthreads();
    if (t == 0) {
        for (int w = 1; w < 4; ++w) {
            nbg += red[0][w];
            nrms += red[1][w];
            kmin = red[2][w] < kmin ? red[2][w] : kmin;
            kmax = red[3][w] > kmax ? red[3][w] : kmax;
            rounds = red[4][w] > rounds ? red[4][w] : rounds;
        }
        const double nan = __builtin_nan("");
        stats[0] = (double)m.G;
        stats[1] = (double)nbg;
        stats[2] = (double)nrms;
        stats[3] = nrms ? ordered_value(kmin) : nan;
        stats[4] = nrms ? ordered_value(kmax) : nan;
        stats[5] = mode != 0 ? (double)*counter : 0.0;
        stats[6] = (double)rounds;
        stats[7] = 0.0;
    }
}

int64_t mesh_nodes(int64_t N, int64_t border, int64_t step)
{
    if (N < 1 || border < 0 || 2 * border >= N || step < 1) return GRIDHIP_EINVAL;
    const int64_t G = (N - 2 * border) / step;
    return G > 1 ? G : 1;
}

struct NmArgs {
    int64_t N;
    const double *image;
    const uint8_t *mask;
    int exclude;
    int64_t border, step, half;
    double kappa;
    int64_t nclip, min_count;
    int mode;
    double *nodes, *background, *rms, *out, *stats;
};

int noise_map_check(gridhip_ctx *ctx, const NmArgs &a)
{
    const double inf = __builtin_inf();
    if (a.N < 1 || a.border < 0 || 2 * a.border >= a.N || a.step < 1 || a.half < 1 || !(a.kappa > 0.0) || !(a.kappa < inf) ||
        a.nclip < 0 || a.nclip > 8 || a.min_count < 1 || (a.exclude != 0 && a.exclude != 1) || a.mode < 0 || a.mode > 2 ||
        !a.image || !a.stats || (a.mode != 0 && !a.out))
        return fail(ctx, GRIDHIP_EINVAL, "noise_map: bad argument");
    if (a.N <= CLEAN_MAX_N) {  // (the byte counts below cannot overflow)
        const size_t cells = (size_t)a.N * a.N;
        const int64_t G = mesh_nodes(a.N, a.border, a.step);
        const size_t nb = (size_t)G * G * 32;
        if (outputs_clash({{a.out, cells * 8}, {a.nodes, nb}, {a.background, cells * 8}, {a.rms, cells * 8}, {a.stats, 64}},
                          {{a.image, cells * 8}, {a.mask, cells}}, {{0, 0}}))
            return fail(ctx, GRIDHIP_EINVAL, "noise_map: only out may be the image itself; nothing else may overlap");
    }
    if (a.half > NM_MAX_HALF) return fail(ctx, GRIDHIP_EUNSUPPORTED, "noise_map: half above %lld", (long long)NM_MAX_HALF);
    if (a.N > CLEAN_MAX_N) return fail(ctx, GRIDHIP_EUNSUPPORTED, "noise_map: N above %lld", (long long)CLEAN_MAX_N);
    return GRIDHIP_OK;
}

// gridhip_noise_map_dev on checked arguments: three kernels on ctx->stream; scratch: the counter, then (when the caller
// keeps no node table) the table
int noise_map_run(gridhip_ctx *ctx, const NmArgs &a, void *scratch)
{
    const NmMesh m{a.N, a.border, a.step, a.N - 2 * a.border, mesh_nodes(a.N, a.border, a.step)};
    u64 *counter = reinterpret_cast<u64 *>(scratch);
    double *nodes = a.nodes ? a.nodes : reinterpret_cast<double *>(reinterpret_cast<char *>(scratch) + 64);
    const int strat = (int)(ctx->img->noisemap_hist & 7);
    const int64_t side = 2 * a.half + 1, cells = side * side;
    // small windows keep several work-groups on a CU; the full window is alone there and takes all 16 waves
    const int block = cells <= 33 * 33 ? 256 : cells <= 65 * 65 ? 512 : 1024;
    const size_t lds = (size_t)cells * 8 + (size_t)((strat & 2) ? block / 64 : 1) * 1024;
    if (!ctx->img->noisemap_lds_raised) {  // (a work-group may take more than 64 KB only once the function is told so)
        GH_CHECK_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(nm_node_kernel),
                                              hipFuncAttributeMaxDynamicSharedMemorySize,
                                              (int)((2 * NM_MAX_HALF + 1) * (2 * NM_MAX_HALF + 1) * 8 + NM_MAX_WAVES * 1024)));
        ctx->img->noisemap_lds_raised = true;
    }
    const int64_t G2 = m.G * m.G, most = (int64_t)ctx->num_cu * 64;
    hipLaunchKernelGGL(nm_node_kernel, dim3((unsigned)(G2 < most ? G2 : most)), dim3(block), lds, ctx->stream, m, a.half,
                       a.image, a.mask, a.exclude, a.kappa, (int)a.nclip, a.min_count, strat, nodes, counter);
    const dim3 mgrid((unsigned)((a.N + 255) / 256), (unsigned)((a.N + NM_MAP_ROWS - 1) / NM_MAP_ROWS));
    hipLaunchKernelGGL(nm_map_kernel, mgrid, dim3(256), 0, ctx->stream, m, a.image, (const double *)nodes, a.mode,
                       a.background, a.rms, a.out, counter);
    hipLaunchKernelGGL(nm_stats_kernel, dim3(1), dim3(256), 0, ctx->stream, m, (const double *)nodes, a.mode,
                       (const u64 *)counter, a.stats);
    GH_CHECK_HIP(ctx, hipGetLastError());
    return GRIDHIP_OK;
}

int noise_map_any(gridhip_ctx *ctx, bool dev, NmArgs a)
{
    if (!ctx) return GRIDHIP_EINVAL;
    GH_CHECK(noise_map_check(ctx, a));
    GH_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    const int64_t G = mesh_nodes(a.N, a.border, a.step);
    DevBuf scratch;
    GH_CHECK(scratch.alloc(ctx, 64 + (a.nodes ? 0 : (size_t)G * G * 32)));
    const size_t cells = (size_t)a.N * a.N;
    Staged st(ctx, dev);
    if (a.mode == 0) a.out = nullptr;  // (mode 0 writes no out: the host form must not stage one back)
    if (a.out && a.out == a.image) {
        a.out = st.inout(a.image, a.out, cells * 8);
        a.image = a.out;
    } else {
        a.image = st.in(a.image, cells * 8);
        a.out = st.out(a.out, cells * 8);
    }
    a.mask = st.in(a.mask, cells);
    a.nodes = st.out(a.nodes, (size_t)G * G * 32);
    a.background = st.out(a.background, cells * 8);
    a.rms = st.out(a.rms, cells * 8);
    a.stats = st.out(a.stats, 64);
    GH_CHECK(st.status());
    GH_CHECK(noise_map_run(ctx, a, scratch.p));
    return st.finish();
}

}  // namespace

}  // namespace gridhip

using namespace gridhip;

extern "C" {

int64_t gridhip_noise_map_nodes(int64_t N, int64_t border, int64_t step) { return mesh_nodes(N, border, step); }

int gridhip_noise_map(gridhip_ctx *ctx, int64_t N, const double *image, const uint8_t *mask, int exclude, int64_t border,
                      int64_t step, int64_t half, double kappa, int64_t nclip, int64_t min_count, int mode, double *nodes,
                      double *background, double *rms, double *out, double *stats)
{
    return noise_map_any(ctx, false, NmArgs{N, image, mask, exclude, border, step, half, kappa, nclip, min_count, mode, nodes,
                                            background, rms, out, stats});
}

int gridhip_noise_map_dev(gridhip_ctx *ctx, int64_t N, const double *image, const uint8_t *mask, int exclude, int64_t border,
                          int64_t step, int64_t half, double kappa, int64_t nclip, int64_t min_count, int mode,
                          double *nodes, double *background, double *rms, double *out, double *stats)
{
    return noise_map_any(ctx, true, NmArgs{N, image, mask, exclude, border, step, half, kappa, nclip, min_count, mode, nodes,
                                           background, rms, out, stats});
}

}  // extern "C"
