// What the gain solvers (gaincal.hip, ddcal.hip, jonescal.hip) share: everything of a solve but its rounded arithmetic.
// The packed key of a visibility, the state block of a solve that stops on the device, the fixed-order sum of a work-group,
// rounded complex products, the classes of a visibility, the interval walk of the iteration kernels (gc_walk) and its
// global-table form, the ends of the prepare and update kernels, the kernels that open a solve's state, rotate its gains and
// write its 8 statistics, the argument rules, the host driver of a solve (gc_solve_run) and its entry point (gc_solve_any).
//
// A module hands the templates below a struct M of static members (GcMod, DdMod<D>, JcMod):
//   NS, NG        doubles of sums and complex gains per antenna;  GSTEP: complex gains between two cells of the caller's table
//   UNROLL        of the walk's add loop: 1 where four visibilities' loads hoisted together would spill
//   In            the per-visibility arrays its add reads, by value;  Held: what a lane loads of its 4 visibilities at the
//                 start of a step (GcNoHeld: nothing)
//   load_gains    one interval's gains into LDS as [A][NG];  add: the two-sided sum of one visibility, gains at gp[d * gstride],
//                 sums at rp, rq - the module's rounded operations, as are its prepare, update and final-pass kernels
//   BLOCK, RESIDENT   a fixed work-group size of the walk and how many a CU holds (BLOCK 0: as many as tables fit, 1024 threads)
//   LDS_MOST, RAISE_BIT, walker()   the dynamic LDS its walk kernel must be allowed once per device, 0: none
//   lds_antennas(), planes(c), rules(c), run(ctx, c) and the launches init, prepare, iter, update, final
#pragma once
#include "common.h"
#include "imaging.h"

namespace gridhip {

namespace {

// key = p | q << 21 | t << 42 | used << 63 (A, T <= GC_MAX_TABLE = 2^21 each)
constexpr unsigned long long GC_USED = 1ull << 63;
constexpr unsigned int GC_FIELD = (1u << 21) - 1;
static_assert(GC_MAX_TABLE <= (int64_t)GC_FIELD + 1, "the key's fields hold an antenna and an interval");
__device__ __forceinline__ int gc_key_p(unsigned long long k) { return (int)(k & GC_FIELD); }
__device__ __forceinline__ int gc_key_q(unsigned long long k) { return (int)(k >> 21 & GC_FIELD); }
__device__ __forceinline__ long long gc_key_t(unsigned long long k) { return (long long)(k >> 42 & GC_FIELD); }
__device__ __forceinline__ unsigned long long gc_pack(int64_t p, int64_t q, int64_t t)
{
    return GC_USED | (unsigned long long)p | (unsigned long long)q << 21 | (unsigned long long)t << 42;
}

struct GcState {  // 128 bytes at the head of the small scratch block
    double rel;          // of the last iteration; NaN before the first
    long long iters;     // iterations performed
    long long stopped;   // rel <= tol reached: every later iteration launch returns
    long long unsolved;  // (t, a) whose den was never > 0 (the finish kernel counts them)
    double chi0;         // chi^2 at g = 1
    double used, flagged, dropped;
    double pad[8];
};
constexpr int GC_HEAD = sizeof(GcState) / 8;  // doubles before the partial rows
constexpr int GC_PARTS = 4;                   // chi^2 at g = 1, used, flagged, dropped
constexpr int GC_CU_THREADS = 1024;           // threads of a walk kernel a CU holds (launch bound 1024: 128 VGPRs a lane)
constexpr int64_t GC_CU_LDS = 160 * 1024;

// the sum of x over the work-group's threads (256 or 1024), in a fixed order, in every thread; lds: 16 values
__device__ __forceinline__ double block_sum(double x, double *lds)
{
    for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o);
    __syncthreads();  // (lds may still be read from the last sum)
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = x;
    __syncthreads();
    double s = lds[0];
    for (int w = 1; w < (int)(blockDim.x >> 6); ++w) s += lds[w];
    return s;
}

__device__ __forceinline__ double2 cmul(double2 a, double2 b)
{
#pragma clang fp contract(off)
    return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}
__device__ __forceinline__ double2 cmulc(double2 a, double2 b)  // a * conj(b)
{
#pragma clang fp contract(off)
    return make_double2(a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y);
}
__device__ __forceinline__ double norm2(double2 a)
{
#pragma clang fp contract(off)
    return a.x * a.x + a.y * a.y;
}

// 0: used, 1: flagged, 2: dropped or an autocorrelation; p, q, t are valid for 0
__device__ __forceinline__ int classify(int64_t k, int64_t A, int64_t T, const int64_t *__restrict__ a1,
                                        const int64_t *__restrict__ a2, const int64_t *__restrict__ slot,
                                        const double *__restrict__ wt, int64_t *p, int64_t *q, int64_t *t, double *s)
{
    *s = wt ? wt[k] : 1.0;
    *p = a1[k], *q = a2[k], *t = slot ? slot[k] : 0;
    if (!(*s > 0.0)) return 1;
    if (*p < 0 || *p >= A || *q < 0 || *q >= A || *t < 0 || *t >= T || *p == *q) return 2;
    return 0;
}

// ---- the iteration kernels ----------------------------------------------------------------------------------------------

struct GcNoHeld {  // a module whose add loads its visibility itself
    template <class In>
    __device__ __forceinline__ void load(const In &, int, int64_t, bool)
    {
    }
};

// the plain load_gains: the table is [T][A][NG], count = NG * A
__device__ __forceinline__ void gc_copy_gains(double2 *lg, const double2 *__restrict__ g, long long tn, int count)
{
    for (int a = threadIdx.x, nt = blockDim.x; a < count; a += nt) lg[a] = g[tn * count + a];
}

// the work-group's sums into their rows of the global table, zeros left out; ZERO: the sums start again
template <bool ZERO>
__device__ __forceinline__ void gc_flush(double *acc, double *rows, int count)
{
    for (int a = threadIdx.x, nt = blockDim.x; a < count; a += nt) {
        const double v = acc[a];
        if (v != 0.0) atomicAdd(&rows[a], v);
        if (ZERO) acc[a] = 0.0;
    }
}

// One iteration's sums where one interval's gains and sums fit in LDS.  Work-group b takes the visibilities
// [b * per, (b + 1) * per), per a whole number of chunks, in steps of 4 blockDim.x: thread i holds the keys (and M::Held) of
// base + i + blockDim.x j.  lg [A][NG], acc [A][NS]: the gains and the sums of interval tcur; the global table is the same
// rows, [T][A][NS].  A step whose used visibilities all lie in tcur costs one barrier; otherwise the work-group agrees on
// the lowest interval still pending, flushes, loads that interval's gains and goes on until nothing is pending.
template <class M>
__device__ __forceinline__ void gc_walk(const typename M::In &in, int64_t n, int A, int64_t T, int64_t per,
                                        const unsigned long long *__restrict__ key, const double2 *__restrict__ g,
                                        double *table, const GcState *st, double2 *lg, double *acc)
{
    if (st->stopped) return;
    __shared__ unsigned int tsel;
    constexpr int NS = M::NS, NG = M::NG;
    const int nt = blockDim.x;
    for (int a = threadIdx.x; a < NS * A; a += nt) acc[a] = 0.0;
    const int64_t k0 = (int64_t)blockIdx.x * per, k1 = k0 + per < n ? k0 + per : n;
    long long tcur = -1;
    for (int64_t base = k0; base < k1; base += 4 * nt) {
        unsigned long long kk[4];
        typename M::Held held;
        unsigned int pend = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t k = base + threadIdx.x + (int64_t)nt * j;
            kk[j] = k < k1 ? key[k] : 0ull;
            held.load(in, j, k, k < k1);
            if (kk[j] & GC_USED) pend |= 1u << j;
        }
        for (;;) {
#pragma unroll M::UNROLL
            for (int j = 0; j < 4; ++j) {
                const unsigned long long kj = j == 0 ? kk[0] : j == 1 ? kk[1] : j == 2 ? kk[2] : kk[3];
                if (!(pend >> j & 1u) || gc_key_t(kj) != tcur) continue;
                const int p = gc_key_p(kj), q = gc_key_q(kj);
                M::add(in, held, j, base + threadIdx.x + (int64_t)nt * j, lg + p * NG, lg + q * NG, 1, acc + p * NS,
                       acc + q * NS);
                pend &= ~(1u << j);
            }
            if (!__syncthreads_or(pend != 0)) break;  // (a barrier: every add into tcur's sums is done)
            if (threadIdx.x == 0) tsel = 0xffffffffu;
            __syncthreads();
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (pend >> j & 1u) atomicMin(&tsel, (unsigned int)gc_key_t(kk[j]));
            __syncthreads();
            const long long tn = tsel;
            if (tcur >= 0) gc_flush<true>(acc, table + (size_t)tcur * A * NS, NS * A);
            M::load_gains(lg, g, tn, A, T);
            __syncthreads();
            tcur = tn;
        }
    }
    __syncthreads();
    if (tcur >= 0) gc_flush<false>(acc, table + (size_t)tcur * A * NS, NS * A);
}

// the same sums for any A: gains from global memory, fp64 atomics straight to the table
template <class M>
__device__ __forceinline__ void gc_walk_global(const typename M::In &in, int64_t n, int64_t A, int64_t T,
                                               const unsigned long long *__restrict__ key, const double2 *__restrict__ g,
                                               double *table, const GcState *st)
{
    if (st->stopped) return;
    const int64_t k0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, step = (int64_t)gridDim.x * blockDim.x;
    for (int64_t k = k0; k < n; k += step) {
        const unsigned long long kk = key[k];
        if (!(kk & GC_USED)) continue;
        const int64_t t = gc_key_t(kk), p = t * A + gc_key_p(kk), q = t * A + gc_key_q(kk);
        typename M::Held held;
        held.load(in, 0, k, true);
        M::add(in, held, 0, k, g + p * M::GSTEP, g + q * M::GSTEP, T * A, table + p * M::NS, table + q * M::NS);
    }
}

// ---- the ends of the prepare and update kernels, and the one-work-group kernels -------------------------------------------

// a prepare kernel's row of partial sums: one per work-group, no atomics
__device__ __forceinline__ void gc_prepare_tail(double chi0, unsigned int used, unsigned int flagged, unsigned int dropped,
                                                double *__restrict__ parts, double *lds)
{
    const double r[GC_PARTS] = {chi0, (double)used, (double)flagged, (double)dropped};
    for (int j = 0; j < GC_PARTS; ++j) {
        const double x = block_sum(r[j], lds);
        if (threadIdx.x == 0) parts[(int64_t)blockIdx.x * GC_PARTS + j] = x;
    }
}

// the end of an update kernel (one work-group): d2 = sum |g' - g|^2 and s2 = sum |g'|^2 of the lanes, rel, the stop test
__device__ __forceinline__ void gc_close_iteration(double d2, double s2, double tol, GcState *st, double *lds)
{
#pragma clang fp contract(off)
    d2 = block_sum(d2, lds);
    s2 = block_sum(s2, lds);
    if (threadIdx.x != 0) return;
    const double rel = sqrt(d2 / s2);
    st->rel = rel;
    st->iters += 1;
    if (tol > 0.0 && rel <= tol) st->stopped = 1;
}

// the rows of the prepare pass, thread t adding the rows t, t + 256, ... in order; the state starts
__global__ void __launch_bounds__(256) gaincal_begin_kernel(int nblk, const double *__restrict__ parts, GcState *st)
{
    __shared__ double lds[16];
    double tot[GC_PARTS];
    for (int j = 0; j < GC_PARTS; ++j) {
        double x = 0.0;
        for (int b = threadIdx.x; b < nblk; b += 256) x += parts[(int64_t)b * GC_PARTS + j];
        tot[j] = block_sum(x, lds);
    }
    if (threadIdx.x != 0) return;
    st->rel = __builtin_nan("");
    st->iters = 0, st->stopped = 0, st->unsolved = 0;
    st->chi0 = tot[0], st->used = tot[1], st->flagged = tot[2], st->dropped = tot[3];
}

// where the gains of a cell e = t * A + a lie: plane d of it at g[d * plane + e * cell].  own: every plane is rotated by its
// own reference gain, else all by plane 0's, of which alone the reference antenna's becomes real; skip: planes not touched
struct GcPlanes {
    int planes;
    int64_t plane, cell;
    bool own;
    unsigned int skip;
};

// One work-group of 1024 threads.  rot[d, t] = conj(r) / |r|, r = the gain of plane d of (t, refant), where the reference
// antenna was solved and r is finite and not zero, else 1: every solved gain of the plane and interval is multiplied by it
// (an unsolved one stays exactly what it started from), the reference antenna's own becomes (|r|, 0).  The gains of an
// interval are read (rot) before any is written: a barrier lies between.  unsolved: the (t, a) never solved, once each.
__global__ void __launch_bounds__(1024)
    gc_finish_kernel(int64_t A, int64_t T, GcPlanes lay, int64_t refant, const unsigned int *__restrict__ ever, double2 *g,
                     double2 *__restrict__ rot, GcState *st)
{
#pragma clang fp contract(off)
    __shared__ double lds[16];
    if (refant >= 0) {
        for (int64_t i = threadIdx.x; i < (lay.own ? lay.planes : 1) * T; i += 1024) {
            const int64_t d = i / T, t = i - d * T;
            const double2 r = g[d * lay.plane + (t * A + refant) * lay.cell];
            const double a = sqrt(norm2(r));
            rot[i] = (ever[t * A + refant] && a > 0.0 && a - a == 0.0) ? make_double2(r.x / a, -r.y / a)
                                                                      : make_double2(1.0, 0.0);
        }
        __syncthreads();
    }
    double un = 0.0;
    for (int64_t e = threadIdx.x; e < A * T; e += 1024) {
        if (!ever[e]) {  // unsolved: counted, and its gains stay the bits they started from
            un += 1.0;
            continue;
        }
        if (refant < 0) continue;
        const int64_t t = e / A;
        for (int d = 0; d < lay.planes; ++d) {
            if (lay.skip >> d & 1u) continue;
            const double2 r = rot[lay.own ? d * T + t : t];
            if (r.x == 1.0 && r.y == 0.0) continue;
            double2 *at = g + d * lay.plane + e * lay.cell;
            const double2 go = *at;
            *at = (e - t * A == refant && (lay.own || d == 0)) ? make_double2(sqrt(norm2(go)), 0.0) : cmul(go, r);
        }
    }
    un = block_sum(un, lds);
    if (threadIdx.x == 0) st->unsolved = (long long)un;
}

__global__ void __launch_bounds__(256)
    gaincal_stats_kernel(int nblk, const double *__restrict__ parts, const GcState *st, double *__restrict__ stats)
{
    __shared__ double lds[16];
    double x = 0.0;
    for (int b = threadIdx.x; b < nblk; b += 256) x += parts[b];
    x = block_sum(x, lds);
    if (threadIdx.x != 0) return;
    stats[0] = (double)st->iters;
    stats[1] = st->rel;
    stats[2] = x;
    stats[3] = st->chi0;
    stats[4] = st->used;
    stats[5] = st->flagged;
    stats[6] = st->dropped;
    stats[7] = (double)st->unsolved;
}

// ---- the host side of a solve -------------------------------------------------------------------------------------------

// the rules the solves, the applies and the subtraction share: the sizes, the limit on the table; D: of ddcal.hip alone
inline int shape_check(gridhip_ctx *ctx, const char *who, int64_t n, int64_t A, int64_t T, const int64_t *a1,
                       const int64_t *a2, const int64_t *slot, const int64_t *D = nullptr)
{
    const bool bad = n < 0 || A < 2 || T < 1 || (!slot && T != 1) || (n > 0 && (!a1 || !a2));
    if (D && (bad || *D < 1 || *D > DD_MAX_D))
        return fail(ctx, GRIDHIP_EINVAL, "%s: n >= 0, A >= 2, T >= 1, D in 1..%d, a slot array unless T == 1, a1 and a2", who,
                    DD_MAX_D);
    if (bad) return fail(ctx, GRIDHIP_EINVAL, "%s: n >= 0, A >= 2, T >= 1, a slot array unless T == 1, a1 and a2", who);
    if (A > GC_MAX_TABLE || T > GC_MAX_TABLE || A * T > GC_MAX_TABLE || (D && *D * A * T > GC_MAX_TABLE))
        return fail(ctx, GRIDHIP_EUNSUPPORTED, D ? "%s: D * A * T above %lld" : "%s: A * T above %lld", who,
                    (long long)GC_MAX_TABLE);
    return GRIDHIP_OK;
}

struct GcCall {  // a solve as its entry point gets it.  D: 1 but for ddcal; vis_cal, wt_cal: gaincal's selfcal outputs
    int64_t n, A, T, D;
    const int64_t *a1, *a2, *slot;
    const double *vis, *model_vis, *wt;
    int mode;
    int64_t refant;
    int warm;
    int64_t niter;
    double tol;
    double *gains, *stats, *vis_cal, *wt_cal;
};

struct GcRules {  // a module's name in messages, its highest mode, whether D is an argument, the bytes of vis and model_vis
    const char *who;  // per visibility and of the gains
    int modes;
    bool dd;
    size_t vis, model, gains;
};

inline int gc_solve_check(gridhip_ctx *ctx, const GcRules &r, const GcCall &c)
{
    if (c.n < 0 || c.A < 2 || c.T < 1 || (r.dd && (c.D < 1 || c.D > DD_MAX_D)) || (!c.slot && c.T != 1) ||
        (c.n > 0 && (!c.a1 || !c.a2 || !c.vis || !c.model_vis)) || !c.gains || c.niter < 0 || !(c.tol >= 0.0) || c.mode < 0 ||
        c.mode > r.modes || c.refant >= c.A)
        return fail(ctx, GRIDHIP_EINVAL, "%s: bad argument", r.who);
    GH_CHECK(shape_check(ctx, r.who, c.n, c.A, c.T, c.a1, c.a2, c.slot, r.dd ? &c.D : nullptr));
    const size_t n8 = (size_t)c.n * 8;
    if (overlaps_any({c.gains, r.gains}, {{c.a1, n8}, {c.a2, n8}, {c.slot, n8}, {c.vis, c.n * r.vis},
                                          {c.model_vis, c.n * r.model}, {c.wt, n8}}))
        return fail(ctx, GRIDHIP_EINVAL, "%s: gains must not overlap an input", r.who);
    return GRIDHIP_OK;
}

struct GcWork {  // what the driver allocates and a module's launches use: pair, real: 16 and 8 bytes per visibility
    dim3 sgrid;  // the prepare pass and the final pass: one row of partial sums per work-group
    double *table;
    unsigned int *ever;
    double2 *pair;
    double *real;
    unsigned long long *key;
    double *parts;
    GcState *st;
    double2 *g;
};

// a solve on device arrays: init, prepare, begin, niter x { iter, update }, finish, the final pass, stats
template <class M>
int gc_solve_run(gridhip_ctx *ctx, const GcCall &c)
{
    const int64_t n = c.n, A = c.A, cells = c.A * c.T;
    const GcPlanes lay = M::planes(c);
    const size_t nparts = (size_t)GC_PARTS * ctx->num_cu * 16;
    DevBuf small, table, ever, pair, real, key;
    GH_CHECK(small.alloc(ctx, ((size_t)GC_HEAD + nparts + 2 * (size_t)(lay.own ? lay.planes : 1) * c.T) * 8));
    GH_CHECK(table.alloc(ctx, (size_t)cells * M::NS * 8));
    GH_CHECK(ever.alloc(ctx, (size_t)cells * 4));
    if (n > 0) {
        if (M::PAIR) GH_CHECK(pair.alloc(ctx, (size_t)n * 16));
        GH_CHECK(real.alloc(ctx, (size_t)n * 8));
        GH_CHECK(key.alloc(ctx, (size_t)n * 8));
    }
    GcWork w = {grid_for(ctx, n), table.as<double>(), ever.as<unsigned int>(), pair.as<double2>(), real.as<double>(),
                key.as<unsigned long long>(), small.as<double>() + GC_HEAD, small.as<GcState>(), (double2 *)c.gains};
    double2 *rot = reinterpret_cast<double2 *>(w.parts + nparts);
    const int nblk = n > 0 ? (int)w.sgrid.x : 0;
    M::init(ctx, c, w);
    if (n > 0) M::prepare(ctx, c, w);
    hipLaunchKernelGGL(gaincal_begin_kernel, dim3(1), dim3(256), 0, ctx->stream, nblk, (const double *)w.parts, w.st);
    GH_CHECK_HIP(ctx, hipGetLastError());
    const bool lds = A <= M::lds_antennas();
    const size_t bytes = M::BLOCK ? 0 : (size_t)A * (M::NS + 2 * M::NG) * 8;
    // a CU holds GC_CU_THREADS threads of a dynamic-LDS walk: as many work-groups as tables fit, each the larger for it
    const int fit = lds ? (int)(GC_CU_LDS / (int64_t)(bytes + 64)) : 0;
    const int block = M::BLOCK ? M::BLOCK : fit >= 4 ? 256 : fit >= 2 ? 512 : 1024;
    const int resident = M::BLOCK ? M::RESIDENT : GC_CU_THREADS / block;
    // (more than 64 KB of LDS only once the function is told so)
    if (M::LDS_MOST && lds && n > 0 && c.niter > 0 && !(ctx->img->gain_lds_raised >> M::RAISE_BIT & 1u)) {
        GH_CHECK_HIP(ctx, hipFuncSetAttribute(M::walker(), hipFuncAttributeMaxDynamicSharedMemorySize, (int)M::LDS_MOST));
        ctx->img->gain_lds_raised |= 1u << M::RAISE_BIT;
    }
    // the walk's ranges: whole chunks, and no more work-groups than are resident at once, so that none waits for another
    const int64_t nchunks = (n + GC_CHUNK - 1) / GC_CHUNK, most = (int64_t)ctx->num_cu * resident;
    const int64_t cpw = nchunks > most ? (nchunks + most - 1) / most : 1;
    const int64_t igrid = nchunks > 0 ? (nchunks + cpw - 1) / cpw : 0;
    for (int64_t i = 0; i < c.niter; ++i) {
        if (n > 0) M::iter(ctx, c, w, lds, dim3((unsigned)igrid), dim3(block), bytes, cpw * GC_CHUNK);
        M::update(ctx, c, w);
    }
    hipLaunchKernelGGL(gc_finish_kernel, dim3(1), dim3(1024), 0, ctx->stream, A, c.T, lay, c.refant,
                       (const unsigned int *)w.ever, w.g, rot, w.st);
    if (n > 0) M::final(ctx, c, w);
    if (c.stats)
        hipLaunchKernelGGL(gaincal_stats_kernel, dim3(1), dim3(256), 0, ctx->stream, nblk, (const double *)w.parts,
                           (const GcState *)w.st, c.stats);
    GH_CHECK_HIP(ctx, hipGetLastError());
    return GRIDHIP_OK;
}

// a solve's entry point, on host or device arrays.  M: a module's rules(c) and run(ctx, c)
template <class M>
int gc_solve_any(gridhip_ctx *ctx, bool dev, GcCall c)
{
    if (!ctx) return GRIDHIP_EINVAL;
    const GcRules r = M::rules(c);
    GH_CHECK(gc_solve_check(ctx, r, c));
    GH_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n8 = (size_t)c.n * 8;
    Staged st(ctx, dev);
    c.a1 = st.in(c.a1, n8), c.a2 = st.in(c.a2, n8), c.slot = st.in(c.slot, n8), c.vis = st.in(c.vis, c.n * r.vis);
    c.model_vis = st.in(c.model_vis, c.n * r.model), c.wt = st.in(c.wt, n8);
    c.gains = c.warm ? st.inout(c.gains, c.gains, r.gains) : st.out(c.gains, r.gains);  // (a cold start reads no gains)
    c.stats = st.out(c.stats, 64);
    GH_CHECK(st.status());
    GH_CHECK(M::run(ctx, c));
    return st.finish();
}

}  // namespace

}  // namespace gridhip
