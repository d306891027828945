// What the gain solvers (gaincal.hip, ddcal.hip, jonescal.hip) share: the packed key of a visibility, the state block of a
// solve that stops on the device, the fixed-order sum of a work-group, rounded complex products, the classes of a
// visibility, the two one-work-group kernels that open a solve's state and write its 8 statistics, and the shape rule.
#pragma once
#include "common.h"
#include "imaging.h"

namespace gridhip {

namespace {

// key = p | q << 21 | t << 42 | used << 63 (A, T <= GC_MAX_TABLE = 2^21 each)
constexpr unsigned long long GC_USED = 1ull << 63;
constexpr unsigned int GC_FIELD = (1u << 21) - 1;
static_assert(GC_MAX_TABLE <= (int64_t)GC_FIELD + 1, "the key's fields hold an antenna and an interval");

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

// the rules the solves and the applies of gaincal.hip and jonescal.hip share: the sizes, the limit on the table
inline int shape_check(gridhip_ctx *ctx, const char *who, int64_t n, int64_t A, int64_t T, const int64_t *a1,
                       const int64_t *a2, const int64_t *slot)
{
    if (n < 0 || A < 2 || T < 1 || (!slot && T != 1) || (n > 0 && (!a1 || !a2)))
        return fail(ctx, GRIDHIP_EINVAL, "%s: n >= 0, A >= 2, T >= 1, a slot array unless T == 1, a1 and a2", who);
    if (A > GC_MAX_TABLE || T > GC_MAX_TABLE || A * T > GC_MAX_TABLE)
        return fail(ctx, GRIDHIP_EUNSUPPORTED, "%s: A * T above %lld", who, (long long)GC_MAX_TABLE);
    return GRIDHIP_OK;
}

}  // namespace

}  // namespace gridhip
