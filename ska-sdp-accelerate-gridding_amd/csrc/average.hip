// Phase shift and averaging (include/gridhip.h, "phase shift and averaging"): the two data-reduction steps in front of
// every other one - a visibility stream rotated to another phase centre, and groups of its samples collapsed into one
// weighted sample each.
//
//     shift_kernel         gridhip_phase_shift: one pass; lane k reads u, v, w, vis of visibility k and writes vis' and
//                          (u', v', w') of the same k - in place is element k read before it is written, by the same lane.
//                          shift_one() is the whole rule and is what the fused averaging calls too: the same bits.
//
// One gridhip_average call is five launches, whatever the data hold (four without stats):
//     avg_zero_kernel      zeroes the state block and the per-group tables (a kernel: no memset node)
//     avg_count_kernel     pass A, one read of the stream: the class of every visibility; per group the number of
//                          participants n_g (32-bit atomicAdd) and, per class of columns, the largest biased exponent
//                          field b of the weighted values (32-bit atomicMax)
//     avg_sum_kernel       pass B, a second read: every weighted value as q = (int64) rint(ldexp(y, 1084 - L - b)), added
//                          to the group's 64-bit integer sums (64-bit integer atomicAdd)
//     avg_final_kernel     per group: the sums back to doubles, one rounded division each; groups with a participant and
//                          the largest n_g (32-bit atomics on the state block)
//     avg_stats_kernel     the 8 doubles
// The tables are column-major ([column][G]): a stream whose neighbours lie in neighbouring groups - groups strided by
// the baseline count - puts a wave's 64 adds of one column into 512 contiguous bytes, and avg_final_kernel reads every
// column coalesced.  Where neighbours SHARE a group - a sorted stream, G = 1 - the lanes of a wave that form a run of one
// group are added up by shuffles first (a segmented reduction) and the run's first lane alone goes to memory.  Integer
// adds commute and associate: neither the arrival order nor the pre-aggregation can change a bit.
// Integer atomics only; no floating-point atomic and no sum of doubles anywhere in this file.
#include <math.h>

#include "common.h"
#include "imaging.h"

namespace gridhip {

namespace {

typedef unsigned long long u64;
typedef unsigned int u32;

constexpr int AVG_COLS = 7;    // re, im, u, v, w, x, weight
constexpr int AVG_CLASSES = 4; // vis (re, im), uvw (u, v, w), x, weight: one exponent b per class
constexpr int AVG_BIAS = 1084; // s = AVG_BIAS - L - b: |q| <= 2^(62 - L)

struct AvgState {  // 256 bytes at the head of the scratch block
    u32 cls[5];    // participants, flagged, left out, not finite; [4]: non-finite coordinates seen by the fused shift
    u32 groups;    // groups with a participant
    u32 max_n;     // the largest n_g
    u32 pad[57];
};
static_assert(sizeof(AvgState) == 256, "the state block");

struct AvgLayout {
    size_t state, cnt, bmax, sums, total;
};

size_t round256(size_t x) { return (x + 255) & ~(size_t)255; }

AvgLayout layout(int64_t G)
{
    AvgLayout l;
    l.state = 0;
    l.cnt = sizeof(AvgState);
    l.bmax = l.cnt + round256((size_t)G * 4);
    l.sums = l.bmax + round256((size_t)G * 4 * AVG_CLASSES);
    l.total = l.sums + round256((size_t)G * 8 * AVG_COLS);
    return l;
}

// the rotation of a call: R row-major, and n0 - 1 of the new centre (l0, m0) = (R[6], R[7]) without the cancellation
struct Shift {
    double r[9];
    double nm1;
};

__device__ __forceinline__ bool is_fin(double x) { return x - x == 0.0; }

// The whole phase-shift rule for one visibility; returns whether a coordinate was not finite (vis then passes through).
// p and its reduction are gridhip_dft_predict's (dft.hip, add_term) with the opposite sign of the exponent.
__device__ __forceinline__ bool shift_one(const Shift &S, double &u, double &v, double &w, double2 &vis)
{
#pragma clang fp contract(off)
    const bool bad = !(is_fin(u) && is_fin(v) && is_fin(w));
    if (!bad) {
        const double p = fma(w, S.nm1, fma(v, S.r[7], u * S.r[6]));
        const double r = p - rint(p);
        double sn, cs;
        sincospi(2.0 * r, &sn, &cs);
        const double a = vis.x * cs, b = vis.y * sn, c = vis.x * sn, d = vis.y * cs;
        vis = make_double2(a - b, c + d);
    }
    const double u0 = u, v0 = v, w0 = w;
    double t;
    t = S.r[0] * u0 + S.r[1] * v0;
    u = t + S.r[2] * w0;
    t = S.r[3] * u0 + S.r[4] * v0;
    v = t + S.r[5] * w0;
    t = S.r[6] * u0 + S.r[7] * v0;
    w = t + S.r[8] * w0;
    return bad;
}

// the sum of x over the work-group's waves goes to *dst with one integer atomic per wave
__device__ __forceinline__ void wave_count(u32 x, u32 *dst)
{
    for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o);
    if ((threadIdx.x & 63) == 0 && x) atomicAdd(dst, x);
}

// vis_out may be vis_in and u_out (v_out, w_out) may be u (v, w): no __restrict__ on those.  u_out == nullptr: no
// coordinate outputs.  bad[0] counts the visibilities whose coordinates are not finite (zeroed by the first launch).
__global__ void __launch_bounds__(256) shift_zero_kernel(u32 *bad) { if (threadIdx.x == 0 && blockIdx.x == 0) bad[0] = 0u; }

__global__ void __launch_bounds__(256)
    shift_kernel(int64_t n, Shift S, const double *u, const double *v, const double *w, int64_t stride, const double2 *vis_in,
                 double2 *vis_out, double *u_out, double *v_out, double *w_out, int64_t out_stride, u32 *bad)
{
    const int64_t k0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, step = (int64_t)gridDim.x * blockDim.x;
    u32 nbad = 0u;
    for (int64_t k = k0; k < n; k += step) {
        double uu = u[k * stride], vv = v[k * stride], ww = w ? w[k * stride] : 0.0;
        double2 x = vis_in[k];
        nbad += (u32)shift_one(S, uu, vv, ww, x);
        vis_out[k] = x;
        if (u_out) u_out[k * out_stride] = uu, v_out[k * out_stride] = vv, w_out[k * out_stride] = ww;
    }
    if (bad) wave_count(nbad, bad);
}

__global__ void __launch_bounds__(64) shift_stats_kernel(int64_t n, const u32 *bad, double *__restrict__ stats)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    stats[0] = (double)(n - (int64_t)bad[0]);
    stats[1] = (double)bad[0];
    stats[2] = 0.0;
    stats[3] = 0.0;
}

// ---- averaging -------------------------------------------------------------------------------------------------------------
struct AvgIn {  // the stream of a call (device pointers; w, x, wt may be null)
    int64_t n, G;
    const int64_t *group;
    const double *u, *v, *w;
    int64_t stride;
    const double *x;
    const double2 *vis;
    const double *wt;
};

// The class of visibility k (0 participant, 1 flagged, 2 left out, 3 not finite) and, for a participant, its group and
// its seven weighted values, each one rounded product.  SHIFT: the visibility is first taken through shift_one; *badc
// then says whether its coordinates were not finite, for EVERY class - gridhip_phase_shift sees all n.
template <bool SHIFT>
__device__ __forceinline__ int load_one(const AvgIn &in, const Shift &S, int64_t k, int64_t *g, double y[AVG_COLS], bool *badc)
{
#pragma clang fp contract(off)
    const double s = in.wt ? in.wt[k] : 1.0;
    double uu = in.u[k * in.stride], vv = in.v[k * in.stride], ww = in.w ? in.w[k * in.stride] : 0.0;
    double2 vis = in.vis[k];
    *badc = false;
    if (SHIFT) *badc = shift_one(S, uu, vv, ww, vis);
    if (!(s > 0.0)) return 1;
    const int64_t gg = in.group ? in.group[k] : 0;
    if (gg < 0 || gg >= in.G) return 2;
    const double xx = in.x ? in.x[k] : 0.0;
    y[0] = s * vis.x, y[1] = s * vis.y, y[2] = s * uu, y[3] = s * vv, y[4] = s * ww, y[5] = s * xx, y[6] = s;
    bool fin = true;
#pragma unroll
    for (int c = 0; c < AVG_COLS; ++c) fin = fin && is_fin(y[c]);
    if (!fin) return 3;
    *g = gg;
    return 0;
}

// Runs of one group inside a wave.  g: the lane's group, or -1 for a lane that adds nothing (it is a run of its own).
// *head: the lane is the first of its run; returns a mask whose bit j says that lane + 2^j lies in the same run - what
// run_sum needs for its step j.  *any: some run of the wave is longer than one lane (wave-uniform).
__device__ __forceinline__ u32 run_mask(int64_t g, int lane, bool *head, bool *any)
{
    const int64_t prev = __shfl_up((long long)g, 1);
    *head = lane == 0 || g < 0 || prev != g;
    *any = __ballot(!*head) != 0ull;
    if (!*any) return 0u;
    int start = *head ? lane : 0;
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(start, o);
        if (lane >= o && t > start) start = t;
    }
    u32 take = 0u;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        const int t = __shfl_down(start, 1 << j);
        if (lane + (1 << j) < 64 && t == start) take |= 1u << j;
    }
    return take;
}

// after step j a lane holds op over the lanes [lane, lane + 2^(j+1)) of its own run; the run's first lane ends with all
template <typename T, typename Op>
__device__ __forceinline__ T run_reduce(T x, u32 take, Op op)
{
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        const T o = __shfl_down(x, 1 << j);
        if (take & (1u << j)) x = op(x, o);
    }
    return x;
}

__device__ __forceinline__ u32 exp_field(double y) { return (u32)((__builtin_bit_cast(u64, y) >> 52) & 0x7ffu); }

__global__ void __launch_bounds__(256) avg_zero_kernel(int64_t quads, uint4 *__restrict__ scratch)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, step = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = t; i < quads; i += step) scratch[i] = make_uint4(0u, 0u, 0u, 0u);
}

// Pass A.  A wave takes 64 consecutive visibilities at a time (the loop bound is wave-uniform: the shuffles of the run
// reduction need every lane).
template <bool SHIFT>
__global__ void __launch_bounds__(256)
    avg_count_kernel(AvgIn in, Shift S, AvgState *st, u32 *__restrict__ cnt, u32 *__restrict__ bmax)
{
    const int lane = threadIdx.x & 63;
    const int64_t step = (int64_t)gridDim.x * blockDim.x;
    u32 c[5] = {0u, 0u, 0u, 0u, 0u};
    for (int64_t kb = (int64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63); kb < in.n; kb += step) {
        const int64_t k = kb + lane;
        int64_t g = -1;
        u32 e[AVG_CLASSES] = {0u, 0u, 0u, 0u}, one = 0u;
        if (k < in.n) {
            double y[AVG_COLS];
            bool badc;
            const int cl = load_one<SHIFT>(in, S, k, &g, y, &badc);
            c[cl] += 1u;
            c[4] += (u32)badc;
            if (cl == 0) {
                one = 1u;
#pragma unroll
                for (int j = 0; j < AVG_COLS; ++j) {
                    const u32 f = exp_field(y[j]);
                    const int q = j < 2 ? 0 : j < 5 ? 1 : j - 3;
                    e[q] = f > e[q] ? f : e[q];
                }
            } else {
                g = -1;
            }
        }
        bool head, any;
        const u32 take = run_mask(g, lane, &head, &any);
        if (any) {
            one = run_reduce(one, take, [](u32 a, u32 b) { return a + b; });
#pragma unroll
            for (int q = 0; q < AVG_CLASSES; ++q) e[q] = run_reduce(e[q], take, [](u32 a, u32 b) { return a > b ? a : b; });
        }
        if (g >= 0 && head) {
            atomicAdd(&cnt[g], one);
#pragma unroll
            for (int q = 0; q < AVG_CLASSES; ++q)
                if (e[q]) atomicMax(&bmax[(int64_t)q * in.G + g], e[q]);
        }
    }
    for (int j = 0; j < 5; ++j) wave_count(c[j], &st->cls[j]);
}

__device__ __forceinline__ int log2_ceil(u32 n) { return n <= 1u ? 0 : 32 - __clz((int)(n - 1u)); }

// Pass B
template <bool SHIFT>
__global__ void __launch_bounds__(256)
    avg_sum_kernel(AvgIn in, Shift S, const u32 *__restrict__ cnt, const u32 *__restrict__ bmax, u64 *__restrict__ sums)
{
    const int lane = threadIdx.x & 63;
    const int64_t step = (int64_t)gridDim.x * blockDim.x;
    for (int64_t kb = (int64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63); kb < in.n; kb += step) {
        const int64_t k = kb + lane;
        int64_t g = -1;
        long long q[AVG_COLS] = {0, 0, 0, 0, 0, 0, 0};
        if (k < in.n) {
            double y[AVG_COLS];
            bool badc;
            if (load_one<SHIFT>(in, S, k, &g, y, &badc) == 0) {
                const int L = log2_ceil(cnt[g]);
                int s[AVG_CLASSES];
#pragma unroll
                for (int c = 0; c < AVG_CLASSES; ++c) s[c] = AVG_BIAS - L - (int)bmax[(int64_t)c * in.G + g];
#pragma unroll
                for (int j = 0; j < AVG_COLS; ++j) q[j] = (long long)rint(ldexp(y[j], s[j < 2 ? 0 : j < 5 ? 1 : j - 3]));
            } else {
                g = -1;
            }
        }
        bool head, any;
        const u32 take = run_mask(g, lane, &head, &any);
        if (any) {
#pragma unroll
            for (int j = 0; j < AVG_COLS; ++j) q[j] = run_reduce(q[j], take, [](long long a, long long b) { return a + b; });
        }
        if (g >= 0 && head) {
#pragma unroll
            for (int j = 0; j < AVG_COLS; ++j)
                if (q[j]) atomicAdd(&sums[(int64_t)j * in.G + g], (u64)q[j]);
        }
    }
}

// one thread per group; x_out and count_out may be null
__global__ void __launch_bounds__(256)
    avg_final_kernel(int64_t G, const u32 *__restrict__ cnt, const u32 *__restrict__ bmax, const u64 *__restrict__ sums,
                     double *__restrict__ u_out, double *__restrict__ v_out, double *__restrict__ w_out, int64_t out_stride,
                     double *__restrict__ x_out, double2 *__restrict__ vis_out, double *__restrict__ wt_out,
                     int64_t *__restrict__ count_out, AvgState *st)
{
#pragma clang fp contract(off)
    const int64_t step = (int64_t)gridDim.x * blockDim.x;
    u32 filled = 0u, most = 0u;
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < G; g += step) {
        const u32 ng = cnt[g];
        double o[AVG_COLS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (ng) {
            const int L = log2_ceil(ng);
#pragma unroll
            for (int j = 0; j < AVG_COLS; ++j) {
                const int s = AVG_BIAS - L - (int)bmax[(int64_t)(j < 2 ? 0 : j < 5 ? 1 : j - 3) * G + g];
                o[j] = ldexp((double)(long long)sums[(int64_t)j * G + g], -s);
            }
#pragma unroll
            for (int j = 0; j < AVG_COLS - 1; ++j) o[j] = o[j] / o[6];
            filled += 1u;
            most = ng > most ? ng : most;
        }
        vis_out[g] = make_double2(o[0], o[1]);
        u_out[g * out_stride] = o[2], v_out[g * out_stride] = o[3], w_out[g * out_stride] = o[4];
        if (x_out) x_out[g] = o[5];
        wt_out[g] = o[6];
        if (count_out) count_out[g] = (int64_t)ng;
    }
    wave_count(filled, &st->groups);
    for (int o = 32; o > 0; o >>= 1) {
        const u32 t = __shfl_down(most, o);
        most = t > most ? t : most;
    }
    if ((threadIdx.x & 63) == 0 && most) atomicMax(&st->max_n, most);
}

__global__ void __launch_bounds__(64) avg_stats_kernel(const AvgState *st, double *__restrict__ stats)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    stats[0] = (double)st->groups;
    stats[1] = (double)st->cls[0];
    stats[2] = (double)st->cls[1];
    stats[3] = (double)st->cls[2];
    stats[4] = (double)st->cls[3];
    stats[5] = (double)st->max_n;
    stats[6] = (double)st->cls[4];
    stats[7] = 0.0;
}

// ---- argument rules ----------------------------------------------------------------------------------------------------------
struct Span {  // n elements of 8 * width bytes, `stride` doubles apart
    const void *p;
    int64_t n, stride, width;
};

size_t span_bytes(const Span &a) { return gridhip::span_bytes(a.n, a.stride, a.width); }

// do two arrays share an element?  Columns of one interleaved array (equal strides, bases a whole number of doubles
// apart that is no multiple of the stride) do not; everything else is judged by the byte ranges.
bool collide(const Span &a, const Span &b)
{
    if (!overlap(a.p, span_bytes(a), b.p, span_bytes(b))) return false;
    const uintptr_t x = (uintptr_t)a.p, y = (uintptr_t)b.p;
    if (a.stride == b.stride && a.width == 1 && b.width == 1 && a.stride > 1) {
        const uintptr_t d = x > y ? x - y : y - x;
        if (d % 8 == 0 && (d / 8) % (uintptr_t)a.stride != 0) return false;
    }
    return true;
}

bool same(const Span &a, const Span &b) { return a.p == b.p && a.stride == b.stride; }

// R: finite, R22 > 0, orthonormal to 1e-9; fills S
int rotation_check(gridhip_ctx *ctx, const char *who, const double *R, Shift *S)
{
    for (int i = 0; i < 9; ++i)
        if (!std::isfinite(R[i])) return fail(ctx, GRIDHIP_EINVAL, "%s: R is not finite", who);
    if (!(R[8] > 0.0)) return fail(ctx, GRIDHIP_EINVAL, "%s: R22 must be > 0 (the new centre lies in front of the old one)", who);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const double d = R[3 * i] * R[3 * j] + R[3 * i + 1] * R[3 * j + 1] + R[3 * i + 2] * R[3 * j + 2] - (i == j ? 1.0 : 0.0);
            if (!(fabs(d) <= 1e-9)) return fail(ctx, GRIDHIP_EINVAL, "%s: R is not a rotation (|R R^T - I| above 1e-9)", who);
        }
    for (int i = 0; i < 9; ++i) S->r[i] = R[i];
    const double r2 = R[6] * R[6] + R[7] * R[7], c2 = 1.0 - r2;
    S->nm1 = -r2 / (1.0 + sqrt(c2 > 0.0 ? c2 : 0.0));
    return GRIDHIP_OK;
}

constexpr int64_t AVG_MAX = (int64_t)0x7fffff00;  // 2^31 - 256

int shift_check(gridhip_ctx *ctx, int64_t n, const double *R, const double *u, const double *v, const double *w,
                int64_t stride, const double *vis_in, const double *vis_out, const double *u_out, const double *v_out,
                const double *w_out, int64_t out_stride, const double *stats, Shift *S)
{
    const int nout = (u_out != nullptr) + (v_out != nullptr) + (w_out != nullptr);
    if (n < 0 || !R || (n > 0 && (!u || !v || !vis_in || !vis_out)) || stride < 1 || (nout != 0 && nout != 3) ||
        (nout == 3 && out_stride < 1))
        return fail(ctx, GRIDHIP_EINVAL, "phase_shift: n >= 0, R, u, v, vis_in, vis_out, strides >= 1, coordinate outputs all or none");
    GH_CHECK(rotation_check(ctx, "phase_shift", R, S));
    if (n < AVG_MAX) {  // (sizes that overflow nothing)
        const Span in[4] = {{u, n, stride, 1}, {v, n, stride, 1}, {w, n, stride, 1}, {vis_in, n, 2, 2}};
        const Span out[5] = {{u_out, n, out_stride, 1}, {v_out, n, out_stride, 1}, {w_out, n, out_stride, 1},
                             {vis_out, n, 2, 2}, {stats, 4, 1, 1}};
        for (int o = 0; o < 5; ++o) {
            for (int i = 0; i < 4; ++i)
                if (!(o == i && same(out[o], in[i])) && collide(out[o], in[i]))
                    return fail(ctx, GRIDHIP_EINVAL, "phase_shift: an output overlaps an input (vis_out may be vis_in, u_out u, "
                                                     "v_out v, w_out w at the same stride)");
            for (int q = o + 1; q < 5; ++q)
                if (collide(out[o], out[q])) return fail(ctx, GRIDHIP_EINVAL, "phase_shift: two outputs overlap");
        }
    }
    if (n >= AVG_MAX) return fail(ctx, GRIDHIP_EUNSUPPORTED, "phase_shift: n must be < 2^31 - 256 per call");
    return GRIDHIP_OK;
}

int shift_run(gridhip_ctx *ctx, int64_t n, const Shift &S, const double *u, const double *v, const double *w, int64_t stride,
              const double *vis_in, double *vis_out, double *u_out, double *v_out, double *w_out, int64_t out_stride,
              double *stats)
{
    DevBuf bad;
    if (stats) {
        GH_CHECK(bad.alloc(ctx, 256));
        hipLaunchKernelGGL(shift_zero_kernel, dim3(1), dim3(256), 0, ctx->stream, bad.as<u32>());
    }
    if (n > 0)
        hipLaunchKernelGGL(shift_kernel, grid_for(ctx, n), dim3(256), 0, ctx->stream, n, S, u, v, w, stride,
                           (const double2 *)vis_in, (double2 *)vis_out, u_out, v_out, w_out, out_stride,
                           stats ? bad.as<u32>() : nullptr);
    if (stats) hipLaunchKernelGGL(shift_stats_kernel, dim3(1), dim3(64), 0, ctx->stream, n, (const u32 *)bad.as<u32>(), stats);
    GH_CHECK_HIP(ctx, hipGetLastError());
    return GRIDHIP_OK;
}

int average_check(gridhip_ctx *ctx, int64_t n, int64_t G, const int64_t *group, const double *R, const double *u,
                  const double *v, const double *w, int64_t stride, const double *x, const double *vis, const double *wt,
                  const double *u_out, const double *v_out, const double *w_out, int64_t out_stride, const double *x_out,
                  const double *vis_out, const double *wt_out, const int64_t *count_out, const double *stats, Shift *S)
{
    if (n < 0 || G < 1 || (n > 0 && ((!group && G != 1) || !u || !v || !vis)) || stride < 1 || out_stride < 1 || !u_out ||
        !v_out || !w_out || !vis_out || !wt_out || (x && !x_out))
        return fail(ctx, GRIDHIP_EINVAL, "average: n >= 0, G >= 1, group unless G == 1, u, v, vis, strides >= 1, u_out, v_out, "
                                         "w_out, vis_out, wt_out, and x_out with x");
    if (R) GH_CHECK(rotation_check(ctx, "average", R, S));
    if (n < AVG_MAX && G <= AVG_MAX) {
        const Span in[7] = {{group, n, 1, 1}, {u, n, stride, 1}, {v, n, stride, 1}, {w, n, stride, 1}, {x, n, 1, 1},
                            {vis, n, 2, 2}, {wt, n, 1, 1}};
        const Span out[8] = {{u_out, G, out_stride, 1}, {v_out, G, out_stride, 1}, {w_out, G, out_stride, 1}, {x_out, G, 1, 1},
                             {vis_out, G, 2, 2}, {wt_out, G, 1, 1}, {count_out, G, 1, 1}, {stats, 8, 1, 1}};
        for (int o = 0; o < 8; ++o) {
            for (int i = 0; i < 7; ++i)
                if (collide(out[o], in[i])) return fail(ctx, GRIDHIP_EINVAL, "average: an output overlaps an input");
            for (int q = o + 1; q < 8; ++q)
                if (collide(out[o], out[q])) return fail(ctx, GRIDHIP_EINVAL, "average: two outputs overlap");
        }
    }
    if (n >= AVG_MAX) return fail(ctx, GRIDHIP_EUNSUPPORTED, "average: n must be < 2^31 - 256 per call");
    if (G > AVG_MAX) return fail(ctx, GRIDHIP_EUNSUPPORTED, "average: G must be <= 2^31 - 256");
    return GRIDHIP_OK;
}

size_t average_scratch_bytes(int64_t G) { return layout(G).total; }

int average_run(gridhip_ctx *ctx, int64_t n, int64_t G, const int64_t *group, const Shift *S, const double *u, const double *v,
                const double *w, int64_t stride, const double *x, const double *vis, const double *wt, double *u_out,
                double *v_out, double *w_out, int64_t out_stride, double *x_out, double *vis_out, double *wt_out,
                int64_t *count_out, double *stats, void *scratch)
{
    const AvgLayout l = layout(G);
    char *base = reinterpret_cast<char *>(scratch);
    AvgState *st = reinterpret_cast<AvgState *>(base + l.state);
    u32 *cnt = reinterpret_cast<u32 *>(base + l.cnt), *bmax = reinterpret_cast<u32 *>(base + l.bmax);
    u64 *sums = reinterpret_cast<u64 *>(base + l.sums);
    const AvgIn in = {n, G, group, u, v, w, stride, x, (const double2 *)vis, wt};
    const Shift none = {{1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}, 0.0};
    const dim3 sgrid = grid_for(ctx, n);
    hipLaunchKernelGGL(avg_zero_kernel, grid_for(ctx, (int64_t)(l.total / 16)), dim3(256), 0, ctx->stream,
                       (int64_t)(l.total / 16), reinterpret_cast<uint4 *>(base));
    if (S) {
        hipLaunchKernelGGL(avg_count_kernel<true>, sgrid, dim3(256), 0, ctx->stream, in, *S, st, cnt, bmax);
        hipLaunchKernelGGL(avg_sum_kernel<true>, sgrid, dim3(256), 0, ctx->stream, in, *S, (const u32 *)cnt, (const u32 *)bmax, sums);
    } else {
        hipLaunchKernelGGL(avg_count_kernel<false>, sgrid, dim3(256), 0, ctx->stream, in, none, st, cnt, bmax);
        hipLaunchKernelGGL(avg_sum_kernel<false>, sgrid, dim3(256), 0, ctx->stream, in, none, (const u32 *)cnt, (const u32 *)bmax,
                           sums);
    }
    hipLaunchKernelGGL(avg_final_kernel, grid_for(ctx, G), dim3(256), 0, ctx->stream, G, (const u32 *)cnt, (const u32 *)bmax,
                       (const u64 *)sums, u_out, v_out, w_out, out_stride, x_out, (double2 *)vis_out, wt_out, count_out, st);
    if (stats) hipLaunchKernelGGL(avg_stats_kernel, dim3(1), dim3(64), 0, ctx->stream, (const AvgState *)st, stats);
    GH_CHECK_HIP(ctx, hipGetLastError());
    return GRIDHIP_OK;
}

}  // namespace

}  // namespace gridhip

using namespace gridhip;

namespace {

int phase_shift_any(gridhip_ctx *ctx, bool dev, int64_t n, const double *R, const double *u, const double *v, const double *w,
                    int64_t uv_stride, const double *vis_in, double *vis_out, double *u_out, double *v_out, double *w_out,
                    int64_t out_stride, double *stats)
{
    if (!ctx) return GRIDHIP_EINVAL;
    Shift S;
    GH_CHECK(shift_check(ctx, n, R, u, v, w, uv_stride, vis_in, vis_out, u_out, v_out, w_out, out_stride, stats, &S));
    GH_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    const size_t sb = span_bytes(n, uv_stride), n8 = (size_t)n * 8;
    Staged st(ctx, dev);
    u = st.in(u, sb), v = st.in(v, sb), w = st.in(w, sb);
    double *dvis = st.inout(vis_in, vis_out, 2 * n8);
    if (!dev) vis_in = dvis;  // (the device copy of vis is shifted in place)
    // (the coordinate outputs are contiguous in their staged blocks and strided at the caller's)
    double *du = st.raw(u_out, n8), *dv = st.raw(v_out, n8), *dw = st.raw(w_out, n8);
    double *dst = st.out(stats, 32);
    GH_CHECK(st.status());
    GH_CHECK(shift_run(ctx, n, S, u, v, w, uv_stride, vis_in, dvis, du, dv, dw, dev ? out_stride : 1, dst));
    if (!dev && u_out) {
        GH_CHECK(download_strided(ctx, u_out, out_stride, du, n));
        GH_CHECK(download_strided(ctx, v_out, out_stride, dv, n));
        GH_CHECK(download_strided(ctx, w_out, out_stride, dw, n));
    }
    return st.finish();
}

int average_any(gridhip_ctx *ctx, bool dev, int64_t n, int64_t G, const int64_t *group, const double *R, const double *u,
                const double *v, const double *w, int64_t uv_stride, const double *x, const double *vis, const double *wt,
                double *u_out, double *v_out, double *w_out, int64_t out_stride, double *x_out, double *vis_out,
                double *wt_out, int64_t *count_out, double *stats)
{
    if (!ctx) return GRIDHIP_EINVAL;
    Shift S;
    GH_CHECK(average_check(ctx, n, G, group, R, u, v, w, uv_stride, x, vis, wt, u_out, v_out, w_out, out_stride, x_out, vis_out,
                           wt_out, count_out, stats, &S));
    GH_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    const size_t sb = span_bytes(n, uv_stride), n8 = (size_t)n * 8, g8 = (size_t)G * 8;
    DevBuf scratch;
    GH_CHECK(scratch.alloc(ctx, average_scratch_bytes(G)));
    Staged st(ctx, dev);
    group = st.in(group, n8), u = st.in(u, sb), v = st.in(v, sb), w = st.in(w, sb), x = st.in(x, n8);
    vis = st.in(vis, 2 * n8), wt = st.in(wt, n8);
    // (the coordinate outputs are contiguous in their staged blocks and strided at the caller's)
    double *du = st.raw(u_out, g8), *dv = st.raw(v_out, g8), *dw = st.raw(w_out, g8);
    double *dx = st.out(x_out, g8), *dvis = st.out(vis_out, 2 * g8), *dwt = st.out(wt_out, g8);
    int64_t *dcnt = st.out(count_out, g8);
    double *dst = st.out(stats, 64);
    GH_CHECK(st.status());
    GH_CHECK(average_run(ctx, n, G, group, R ? &S : nullptr, u, v, w, uv_stride, x, vis, wt, du, dv, dw, dev ? out_stride : 1, dx,
                         dvis, dwt, dcnt, dst, scratch.p));
    if (!dev) {
        GH_CHECK(download_strided(ctx, u_out, out_stride, du, G));
        GH_CHECK(download_strided(ctx, v_out, out_stride, dv, G));
        GH_CHECK(download_strided(ctx, w_out, out_stride, dw, G));
    }
    return st.finish();
}

}  // namespace

extern "C" {

int gridhip_phase_shift_dev(gridhip_ctx *ctx, int64_t n, const double *R, const double *u, const double *v, const double *w,
                            int64_t uv_stride, const double *vis_in, double *vis_out, double *u_out, double *v_out,
                            double *w_out, int64_t out_stride, double *stats)
{
    return phase_shift_any(ctx, true, n, R, u, v, w, uv_stride, vis_in, vis_out, u_out, v_out, w_out, out_stride, stats);
}

int gridhip_phase_shift(gridhip_ctx *ctx, int64_t n, const double *R, const double *u, const double *v, const double *w,
                        int64_t uv_stride, const double *vis_in, double *vis_out, double *u_out, double *v_out, double *w_out,
                        int64_t out_stride, double *stats)
{
    return phase_shift_any(ctx, false, n, R, u, v, w, uv_stride, vis_in, vis_out, u_out, v_out, w_out, out_stride, stats);
}

int gridhip_average_dev(gridhip_ctx *ctx, int64_t n, int64_t G, const int64_t *group, const double *R, const double *u,
                        const double *v, const double *w, int64_t uv_stride, const double *x, const double *vis,
                        const double *wt, double *u_out, double *v_out, double *w_out, int64_t out_stride, double *x_out,
                        double *vis_out, double *wt_out, int64_t *count_out, double *stats)
{
    return average_any(ctx, true, n, G, group, R, u, v, w, uv_stride, x, vis, wt, u_out, v_out, w_out, out_stride, x_out, vis_out,
                       wt_out, count_out, stats);
}

int gridhip_average(gridhip_ctx *ctx, int64_t n, int64_t G, const int64_t *group, const double *R, const double *u,
                    const double *v, const double *w, int64_t uv_stride, const double *x, const double *vis, const double *wt,
                    double *u_out, double *v_out, double *w_out, int64_t out_stride, double *x_out, double *vis_out,
                    double *wt_out, int64_t *count_out, double *stats)
{
    return average_any(ctx, false, n, G, group, R, u, v, w, uv_stride, x, vis, wt, u_out, v_out, w_out, out_stride, x_out, vis_out,
                       wt_out, count_out, stats);
}

}  // extern "C"
