// Continuum subtraction (include/gridhip.h, "continuum subtraction"): a Chebyshev polynomial of degree D <= 3 along the
// channel axis, fitted per row (spectrum) to the line-free, unflagged samples by weighted least squares, with up to four
// clip rounds, then subtracted or written out as the model.
//
// One call is three launches whatever the data hold:
//     cs_prologue_kernel      the table T_p[c], p <= 2D, and the effective channel mask, [C][8] doubles; the 8 counters zeroed
//     cs_main_kernel<L, N, D> a lane owns a row through all passes: moments, solve, per clip round the residual sum then
//                             clip + moments + solve, then the closing pass that writes `out`
//     cs_stats_kernel         the 8 counters as doubles
//
// THE MAIN KERNEL.  Every floating-point sum belongs to one lane, which walks its row in channel order; only how a sample
// reaches its lane differs between the layouts, so both give the same bits.
//   layout 1, [C][R]: lane r reads data[c R + r] - consecutive lanes, consecutive addresses - straight from global
//     memory, CS_BLOCK channels loaded ahead of their use (`out` may be `data`, so the compiler cannot move a load over a
//     store itself; a sample is only ever rewritten by the lane that read it).
//   layout 0, [R][C]: a work-group of one wave owns CS_ROWS rows and streams chunks of CS_CHUNK channels through LDS:
//     the loads run along the channel (a row's chunk is 128 or 256 contiguous bytes) into registers, one chunk ahead of
//     the one being walked, and go to LDS when that walk is done; then lane l walks row l of the staged chunk.  The staged row pitch is CS_CHUNK + 1 samples: 17 x 16 B for complex samples, read with ds_read_b128,
//     whose 16-lane groups then cover all sixteen 16-byte slots of the 256-byte bank row once; 17 x 8 B for real samples
//     and for the weights, read with ds_read_b64, whose 32-lane groups cover the 32 bank pairs once.  The closing pass puts
//     its results back into the staged chunk and the work-group stores them along the channel.
//   T_p[c] and the channel's state are the same for every lane: one 64-byte row per channel, read through a pointer the
//   compiler knows to be unaliased, so that it may use scalar loads.
//   The clip state of a sample is its byte in `codes` (the caller's, or n bytes of scratch when there are clip rounds and
//   the caller passes none), read and written only by the lane that owns the row.  Without clip rounds and without `codes`
//   there is no byte array: the class of a sample is a function of (weight, value, channel) and is formed again in
//   every pass.
//   A row whose round clipped nothing is finished; a wave all of whose rows are finished leaves the round loop.
// Determinism: fixed accumulation chains, contraction off, correctly rounded division; integer atomics for the counters.
#include "common.h"
#include "imaging.h"

#pragma clang fp contract(off)

namespace gridhip {

namespace {

typedef unsigned long long u64;
typedef unsigned int u32;

constexpr int CS_ROWS = 64;               // layout 0: rows of a work-group, one lane each
constexpr int CS_CHUNK = 16;              // layout 0: channels of a staged chunk
constexpr int CS_PITCH = CS_CHUNK + 1;    // the staged row pitch, in samples
constexpr int CS_THREADS1 = 256;          // layout 1: rows of a work-group
constexpr int CS_BLOCK = 4;               // layout 1: channels loaded ahead
constexpr int CS_TAB = 8;                 // doubles per channel of the table: T_0 .. T_6, the channel's state
constexpr int64_t CS_MAX_C = GRIDHIP_CONTSUB_MAX_CHANNELS;
constexpr int64_t CS_MAX_R = 0x7fffffffLL;
static_assert(2 * GRIDHIP_CONTSUB_MAX_DEGREE + 1 < CS_TAB, "a table row holds T_0 .. T_2D and the state");
static_assert(CS_ROWS == 64 && (CS_CHUNK & (CS_CHUNK - 1)) == 0 && CS_PITCH % 2 == 1, "the staging's index arithmetic and pitch");

struct CsArgs {
    int64_t R, C;
    const double *data, *wt;
    double *out, *coeffs, *rowinfo;
    uint8_t *codes;  // the caller's bytes, the call's own, or null (no clip rounds and no caller's bytes)
    u64 *counters;
    double lim;      // nsigma * nsigma
    int niter;       // the clip rounds (0 when nsigma == 0)
    int mode;
};

// the state of channel c in its table row: 1 in the effective mask, 0 outside it, NaN where x[c] is not finite
__global__ void __launch_bounds__(256)
    cs_prologue_kernel(int64_t C, int degree, const double *__restrict__ x, const uint8_t *__restrict__ mask,
                       double *__restrict__ tab, u64 *__restrict__ counters)
{
#pragma clang fp contract(off)
    const int64_t c0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, step = (int64_t)gridDim.x * blockDim.x;
    if (c0 < 8) counters[c0] = 0;
    for (int64_t c = c0; c < C; c += step) {
        const double xv = x[c];
        double t[CS_TAB];
#pragma unroll
        for (int p = 0; p < CS_TAB; ++p) t[p] = 0.0;
        t[0] = 1.0;
        if (degree >= 1) t[1] = xv;
        const double x2 = 2.0 * xv;
#pragma unroll
        for (int p = 1; p < CS_TAB - 2; ++p)
            if (p + 1 <= 2 * degree) t[p + 1] = x2 * t[p] - t[p - 1];
        const bool fin = xv - xv == 0.0;
        t[CS_TAB - 1] = !fin ? __builtin_nan("") : (!mask || mask[c] != 0) ? 1.0 : 0.0;
#pragma unroll
        for (int p = 0; p < CS_TAB; ++p) tab[c * CS_TAB + p] = t[p];
    }
}

__global__ void __launch_bounds__(64) cs_stats_kernel(const u64 *__restrict__ counters, double *__restrict__ stats)
{
    if (stats && threadIdx.x < GRIDHIP_CONTSUB_STATS) stats[threadIdx.x] = (double)counters[threadIdx.x];
}

__device__ __forceinline__ bool cs_finite(double v) { return v - v == 0.0; }

// The fit of one row: the moments and right-hand sides, the LDL^T factors and the coefficients, all in registers (every
// index is a constant once the loops are unrolled).
template <int D, int NC>
struct Fit {
    double mu[2 * D + 1], b[D + 1][NC], L[D + 1][D + 1], d[D + 1], a[D + 1][NC];
    int deg;
    u32 n;

    __device__ __forceinline__ void clear()
    {
#pragma unroll
        for (int p = 0; p <= 2 * D; ++p) mu[p] = 0.0;
#pragma unroll
        for (int k = 0; k <= D; ++k)
#pragma unroll
            for (int e = 0; e < NC; ++e) b[k][e] = 0.0;
        n = 0u;
    }
    __device__ __forceinline__ void add(double w, const double *t, const double (&v)[NC])
    {
#pragma unroll
        for (int p = 0; p <= 2 * D; ++p) mu[p] = mu[p] + w * t[p];
#pragma unroll
        for (int k = 0; k <= D; ++k) {
            const double g = w * t[k];
#pragma unroll
            for (int e = 0; e < NC; ++e) b[k][e] = b[k][e] + g * v[e];
        }
        n += 1u;
    }
    __device__ __forceinline__ double A(int j, int k) const { return 0.5 * (mu[j + k] + mu[j > k ? j - k : k - j]); }
    __device__ __forceinline__ void solve()
    {
        deg = D;
        bool open = true;
#pragma unroll
        for (int k = 0; k <= D; ++k) {
            d[k] = 1.0;
#pragma unroll
            for (int i = 0; i <= D; ++i) L[i][k] = 0.0;
        }
#pragma unroll
        for (int k = 0; k <= D; ++k) {
            if (!open) continue;
            const double akk = A(k, k);
            double t = akk;
#pragma unroll
            for (int p = 0; p < k; ++p) t = t - (L[k][p] * L[k][p]) * d[p];
            if (akk > 0.0 && t > 1e-12 * akk) {
                d[k] = t;
#pragma unroll
                for (int i = k + 1; i <= D; ++i) {
                    double s = A(i, k);
#pragma unroll
                    for (int p = 0; p < k; ++p) s = s - (L[i][p] * L[k][p]) * d[p];
                    L[i][k] = s / t;
                }
            } else {
                deg = k - 1;
                open = false;
            }
        }
        double z[D + 1][NC];
#pragma unroll
        for (int k = 0; k <= D; ++k)
#pragma unroll
            for (int e = 0; e < NC; ++e) {
                double s = b[k][e];
#pragma unroll
                for (int p = 0; p < k; ++p) s = s - L[k][p] * z[p][e];
                z[k][e] = s;
            }
#pragma unroll
        for (int k = D; k >= 0; --k)
#pragma unroll
            for (int e = 0; e < NC; ++e) {
                double s = 0.0;
                if (k <= deg) {
                    s = z[k][e] / d[k];
#pragma unroll
                    for (int i = k + 1; i <= D; ++i)
                        if (i <= deg) s = s - L[i][k] * a[i][e];
                }
                a[k][e] = s;
            }
    }
    __device__ __forceinline__ double continuum(const double *t, int e) const
    {
        double acc = a[0][e];
#pragma unroll
        for (int k = 1; k <= D; ++k) acc = acc + a[k][e] * t[k];
        return acc;
    }
    // q_c = w (r.re r.re + r.im r.im) of the sample's residual
    __device__ __forceinline__ double q(double w, const double *t, const double (&v)[NC]) const
    {
        const double r0 = v[0] - continuum(t, 0);
        if (NC == 1) return w * (r0 * r0);
        const double r1 = v[NC - 1] - continuum(t, NC - 1);
        return w * (r0 * r0 + r1 * r1);
    }
};

// the class of a sample from its weight, its value and its channel's state: 1, 3, 2 or 0
template <int NC>
__device__ __forceinline__ int cs_class(bool weighted, double w, const double (&v)[NC], double state)
{
    if (weighted && !(w > 0.0 && cs_finite(w))) return 1;
    bool fin = true;
#pragma unroll
    for (int e = 0; e < NC; ++e) fin = fin && cs_finite(v[e]);
    if (!fin) return 3;
    return state == 1.0 ? 0 : 2;
}

// Layout 1: lane `r` walks its row of [C][R], CS_BLOCK channels loaded ahead.  f(k, t, v, w) sees sample k = c R + r, the
// table row of its channel, its value (which it may replace: `write` stores it to out) and its weight.
template <int NC, class F>
__device__ __forceinline__ void cs_walk1(const CsArgs &q, const double *__restrict__ tab, int64_t r, bool active, bool write, F f)
{
    if (!active) return;
    for (int64_t c0 = 0; c0 < q.C; c0 += CS_BLOCK) {
        double v[CS_BLOCK][NC], w[CS_BLOCK];
#pragma unroll
        for (int j = 0; j < CS_BLOCK; ++j) {
            const int64_t k = (c0 + j) * q.R + r;
            const bool in = c0 + j < q.C;
#pragma unroll
            for (int e = 0; e < NC; ++e) v[j][e] = in ? q.data[k * NC + e] : 0.0;
            w[j] = in && q.wt ? q.wt[k] : 1.0;
        }
#pragma unroll
        for (int j = 0; j < CS_BLOCK; ++j) {
            if (c0 + j >= q.C) continue;
            const int64_t k = (c0 + j) * q.R + r;
            f(k, tab + (c0 + j) * CS_TAB, v[j], w[j]);
            if (write) {
#pragma unroll
                for (int e = 0; e < NC; ++e) q.out[k * NC + e] = v[j][e];
            }
        }
    }
}

// Layout 0: the work-group's CS_ROWS rows from r0 of [R][C], a chunk of CS_CHUNK channels at a time through LDS.  Every
// lane takes part in the staging whether its own row is `active` or not; a pass that no lane needs is skipped whole.
template <int NC, class F>
__device__ __forceinline__ void cs_walk0(const CsArgs &q, const double *__restrict__ tab, int64_t r0, bool active, bool write,
                                         double *sd, double *sw, F f)
{
    constexpr int W = CS_CHUNK * NC, SD = CS_PITCH * NC;  // doubles of a row's chunk in memory, and staged
    if (!__any(active)) return;
    const int lane = threadIdx.x;
    // A chunk travels global memory -> registers -> LDS: the loads of chunk k + 1 are issued before chunk k is walked and
    // are waited for only after it, so a wave has a whole chunk in flight while it computes.  (A row is rewritten only by
    // this work-group and only after its chunk has been read, so reading ahead of the stores is safe when out == data.)
    double pre[W], prew[CS_CHUNK];
    auto fetch = [&](int64_t c0) {
        const int nch = q.C - c0 < CS_CHUNK ? (int)(q.C - c0) : CS_CHUNK;
#pragma unroll
        for (int i = 0; i < W; ++i) {
            const int idx = i * CS_ROWS + lane, row = idx / W, col = idx % W;
            pre[i] = r0 + row < q.R && col < nch * NC ? q.data[((r0 + row) * q.C + c0) * NC + col] : 0.0;
        }
        if (q.wt) {
#pragma unroll
            for (int i = 0; i < CS_CHUNK; ++i) {
                const int idx = i * CS_ROWS + lane, row = idx / CS_CHUNK, col = idx % CS_CHUNK;
                prew[i] = r0 + row < q.R && col < nch ? q.wt[(r0 + row) * q.C + c0 + col] : 1.0;
            }
        }
    };
    fetch(0);
    for (int64_t c0 = 0; c0 < q.C; c0 += CS_CHUNK) {
        const int nch = q.C - c0 < CS_CHUNK ? (int)(q.C - c0) : CS_CHUNK;
        __syncthreads();  // (the chunk before has been walked and, when written, stored)
#pragma unroll
        for (int i = 0; i < W; ++i) {
            const int idx = i * CS_ROWS + lane, row = idx / W, col = idx % W;
            sd[row * SD + col] = pre[i];
        }
        if (q.wt) {
#pragma unroll
            for (int i = 0; i < CS_CHUNK; ++i) {
                const int idx = i * CS_ROWS + lane, row = idx / CS_CHUNK, col = idx % CS_CHUNK;
                sw[row * CS_PITCH + col] = prew[i];
            }
        }
        __syncthreads();
        if (c0 + CS_CHUNK < q.C) fetch(c0 + CS_CHUNK);
        if (active) {
            const int64_t kb = (r0 + lane) * q.C + c0;
            for (int j = 0; j < nch; ++j) {
                double v[NC];
                if (NC == 2) {
                    const double2 vv = reinterpret_cast<const double2 *>(sd)[lane * CS_PITCH + j];
                    v[0] = vv.x, v[NC - 1] = vv.y;
                } else {
                    v[0] = sd[lane * CS_PITCH + j];
                }
                const double w = q.wt ? sw[lane * CS_PITCH + j] : 1.0;
                f(kb + j, tab + (c0 + j) * CS_TAB, v, w);
                if (write) {
                    if (NC == 2)
                        reinterpret_cast<double2 *>(sd)[lane * CS_PITCH + j] = make_double2(v[0], v[NC - 1]);
                    else
                        sd[lane * CS_PITCH + j] = v[0];
                }
            }
        }
        if (write) {
            __syncthreads();
#pragma unroll 8
            for (int i = 0; i < W; ++i) {
                const int idx = i * CS_ROWS + lane, row = idx / W, col = idx % W;
                if (r0 + row < q.R && col < nch * NC) q.out[((r0 + row) * q.C + c0) * NC + col] = sd[row * SD + col];
            }
        }
    }
}

__device__ __forceinline__ void cs_wave_count(u32 x, u64 *dst)
{
    for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o);
    if ((threadIdx.x & 63) == 0 && x) atomicAdd(dst, (u64)x);
}

template <int LAYOUT, int NC, int D>
__global__ void __launch_bounds__(LAYOUT ? CS_THREADS1 : CS_ROWS) cs_main_kernel(CsArgs q, const double *__restrict__ tab)
{
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(16))) double sd[LAYOUT ? 2 : CS_ROWS * CS_PITCH * NC];
    __shared__ double sw[LAYOUT ? 1 : CS_ROWS * CS_PITCH];
    const int64_t r0 = (int64_t)blockIdx.x * blockDim.x, r = r0 + threadIdx.x;
    const bool valid = r < q.R, weighted = q.wt != nullptr;
    auto walk = [&](bool active, bool write, auto f) {
        if constexpr (LAYOUT != 0)
            cs_walk1<NC>(q, tab, r, active, write, f);
        else
            cs_walk0<NC>(q, tab, r0, active, write, sd, sw, f);
    };
    Fit<D, NC> fit;
    u32 n_flagged = 0u, n_notfinite = 0u, n_clipped = 0u;

    // the classes, and the moments of the participants
    fit.clear();
    walk(valid, false, [&](int64_t k, const double *t, double(&v)[NC], double w) {
        const int cls = cs_class<NC>(weighted, w, v, t[CS_TAB - 1]);
        if (q.codes) q.codes[k] = (uint8_t)cls;
        if (cls == 0) fit.add(w, t, v);
        n_flagged += cls == 1 ? 1u : 0u;
        n_notfinite += cls == 3 ? 1u : 0u;
    });
    fit.solve();

    // the clip rounds: a participant is a sample of class 0 whose byte no earlier round has set
    bool done = !valid || fit.deg < 0;
    for (int i = 0; i < q.niter; ++i) {
        if (__all(done)) break;
        const bool look = i > 0;  // (round 0 meets no clipped sample)
        double Q = 0.0;
        walk(!done, false, [&](int64_t k, const double *t, double(&v)[NC], double w) {
            if (cs_class<NC>(weighted, w, v, t[CS_TAB - 1]) != 0 || (look && q.codes[k] >= 16)) return;
            Q = Q + fit.q(w, t, v);
        });
        const double limit = q.lim * (Q / (double)fit.n);
        u32 hit = 0u;
        if (!done) fit.clear();
        walk(!done, false, [&](int64_t k, const double *t, double(&v)[NC], double w) {
            if (cs_class<NC>(weighted, w, v, t[CS_TAB - 1]) != 0 || (look && q.codes[k] >= 16)) return;
            if (fit.q(w, t, v) > limit) {
                q.codes[k] = (uint8_t)(16 + i);
                hit += 1u;
            } else {
                fit.add(w, t, v);
            }
        });
        if (!done) {
            fit.solve();
            n_clipped += hit;
            done = hit == 0u || fit.deg < 0;
        }
    }

    // the closing pass: out, and the final qbar from the residuals it forms anyway
    double Qf = 0.0;
    const bool look = n_clipped > 0u;
    const double nan = __builtin_nan("");
    walk(valid, true, [&](int64_t k, const double *t, double(&v)[NC], double w) {
        const double state = t[CS_TAB - 1];
        const bool part = cs_class<NC>(weighted, w, v, state) == 0 && !(look && q.codes[k] >= 16);
        double cont[NC], res[NC];
#pragma unroll
        for (int e = 0; e < NC; ++e) {
            cont[e] = fit.continuum(t, e);
            res[e] = v[e] - cont[e];
        }
        if (part) Qf = Qf + (NC == 1 ? w * (res[0] * res[0]) : w * (res[0] * res[0] + res[NC - 1] * res[NC - 1]));
#pragma unroll
        for (int e = 0; e < NC; ++e) v[e] = state != state ? nan : q.mode ? cont[e] : res[e];
    });

    if (valid) {
        if (q.coeffs) {
#pragma unroll
            for (int k = 0; k <= D; ++k)
#pragma unroll
                for (int e = 0; e < NC; ++e) q.coeffs[(LAYOUT ? k * q.R + r : r * (D + 1) + k) * NC + e] = fit.a[k][e];
        }
        if (q.rowinfo) {
            const double info[GRIDHIP_CONTSUB_ROWINFO] = {(double)fit.deg, (double)fit.n, (double)n_clipped,
                                                          fit.n ? Qf / (double)fit.n : nan};
#pragma unroll
            for (int j = 0; j < GRIDHIP_CONTSUB_ROWINFO; ++j) q.rowinfo[LAYOUT ? j * q.R + r : r * GRIDHIP_CONTSUB_ROWINFO + j] = info[j];
        }
    }
    const int deg = fit.deg;
    cs_wave_count(valid ? 1u : 0u, q.counters + 0);
    cs_wave_count(valid && deg == D ? 1u : 0u, q.counters + 1);
    cs_wave_count(valid && deg >= 0 && deg < D ? 1u : 0u, q.counters + 2);
    cs_wave_count(valid && deg < 0 ? 1u : 0u, q.counters + 3);
    cs_wave_count(valid ? fit.n : 0u, q.counters + 4);
    cs_wave_count(valid ? n_clipped : 0u, q.counters + 5);
    cs_wave_count(valid ? n_notfinite : 0u, q.counters + 6);
    cs_wave_count(valid ? n_flagged : 0u, q.counters + 7);
}

template <int LAYOUT, int NC>
void cs_launch(gridhip_ctx *ctx, int degree, const CsArgs &q, const double *tab)
{
    const int threads = LAYOUT ? CS_THREADS1 : CS_ROWS;
    const dim3 grid((unsigned)((q.R + threads - 1) / threads)), block(threads);
    switch (degree) {
        case 0: hipLaunchKernelGGL((cs_main_kernel<LAYOUT, NC, 0>), grid, block, 0, ctx->stream, q, tab); break;
        case 1: hipLaunchKernelGGL((cs_main_kernel<LAYOUT, NC, 1>), grid, block, 0, ctx->stream, q, tab); break;
        case 2: hipLaunchKernelGGL((cs_main_kernel<LAYOUT, NC, 2>), grid, block, 0, ctx->stream, q, tab); break;
        default: hipLaunchKernelGGL((cs_main_kernel<LAYOUT, NC, 3>), grid, block, 0, ctx->stream, q, tab); break;
    }
}

size_t round256(size_t x) { return (x + 255) & ~(size_t)255; }

int cs_check(gridhip_ctx *ctx, int64_t R, int64_t C, int layout, int ncomp, int degree, int mode, const double *x,
             const uint8_t *chan_mask, const double *data, const double *wt, double nsigma, int64_t niter, const double *out,
             const double *coeffs, const double *rowinfo, const uint8_t *codes, const double *stats)
{
    const bool ok = data && x && out && R >= 1 && C >= 1 && (layout == 0 || layout == 1) && (mode == 0 || mode == 1) &&
                    (ncomp == 1 || ncomp == 2) && degree >= 0 && degree <= GRIDHIP_CONTSUB_MAX_DEGREE && nsigma >= 0.0 &&
                    isfinite(nsigma) && niter >= 0 && niter <= 4;
    if (!ok) return fail(ctx, GRIDHIP_EINVAL, "contsub: bad argument");
    const bool fits = C <= CS_MAX_C && R <= CS_MAX_R;
    if (fits) {  // (sizes that overflow nothing)
        const size_t n = (size_t)(R * C), n8 = n * 8, R8 = (size_t)R * 8;
        const int clash = outputs_clash({{out, n8 * ncomp}, {coeffs, R8 * (degree + 1) * ncomp}, {rowinfo, R8 * GRIDHIP_CONTSUB_ROWINFO},
                                         {codes, n}, {stats, GRIDHIP_CONTSUB_STATS * 8}},
                                        {{data, n8 * ncomp}, {wt, n8}, {x, (size_t)C * 8}, {chan_mask, (size_t)C}}, {{0, 0}});
        if (clash == 1) return fail(ctx, GRIDHIP_EINVAL, "contsub: an output overlaps an input (only out may be data)");
        if (clash == 2) return fail(ctx, GRIDHIP_EINVAL, "contsub: two outputs overlap");
    }
    if (C > CS_MAX_C) return fail(ctx, GRIDHIP_EUNSUPPORTED, "contsub: C above %lld", (long long)CS_MAX_C);
    if (R > CS_MAX_R) return fail(ctx, GRIDHIP_EUNSUPPORTED, "contsub: R above 2^31 - 1");
    return GRIDHIP_OK;
}

int cs_any(gridhip_ctx *ctx, bool dev, int64_t R, int64_t C, int layout, int ncomp, int degree, int mode, const double *x,
           const uint8_t *chan_mask, const double *data, const double *wt, double nsigma, int64_t niter, double *out,
           double *coeffs, double *rowinfo, uint8_t *codes, double *stats)
{
    if (!ctx) return GRIDHIP_EINVAL;
    GH_CHECK(cs_check(ctx, R, C, layout, ncomp, degree, mode, x, chan_mask, data, wt, nsigma, niter, out, coeffs, rowinfo, codes,
                      stats));
    GH_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)(R * C), n8 = n * 8, R8 = (size_t)R * 8;
    const int rounds = nsigma == 0.0 ? 0 : (int)niter;
    // the table and the counters; the call's own bytes only where rounds need them and the caller gives none
    const size_t tab_bytes = round256((size_t)C * CS_TAB * 8);
    DevBuf scratch, bytes;
    GH_CHECK(scratch.alloc(ctx, tab_bytes + 256));
    const bool own = !codes && rounds > 0;
    if (own) GH_CHECK(bytes.alloc(ctx, n));
    Staged sg(ctx, dev);
    x = sg.in(x, (size_t)C * 8), chan_mask = sg.in(chan_mask, (size_t)C);
    data = sg.in(data, n8 * ncomp), wt = sg.in(wt, n8);
    out = sg.out(out, n8 * ncomp), coeffs = sg.out(coeffs, R8 * (degree + 1) * ncomp);
    rowinfo = sg.out(rowinfo, R8 * GRIDHIP_CONTSUB_ROWINFO), codes = sg.out(codes, n), stats = sg.out(stats, GRIDHIP_CONTSUB_STATS * 8);
    GH_CHECK(sg.status());
    double *tab = scratch.as<double>();
    CsArgs q;
    q.R = R, q.C = C, q.data = data, q.wt = wt, q.out = out, q.coeffs = coeffs, q.rowinfo = rowinfo;
    q.codes = own ? bytes.as<uint8_t>() : codes;
    q.counters = reinterpret_cast<u64 *>(scratch.as<char>() + tab_bytes);
    q.lim = nsigma * nsigma, q.niter = rounds, q.mode = mode;
    hipLaunchKernelGGL(cs_prologue_kernel, grid_for(ctx, C), dim3(256), 0, ctx->stream, C, degree, x, chan_mask, tab, q.counters);
    if (layout == 0) {
        if (ncomp == 1)
            cs_launch<0, 1>(ctx, degree, q, tab);
        else
            cs_launch<0, 2>(ctx, degree, q, tab);
    } else {
        if (ncomp == 1)
            cs_launch<1, 1>(ctx, degree, q, tab);
        else
            cs_launch<1, 2>(ctx, degree, q, tab);
    }
    hipLaunchKernelGGL(cs_stats_kernel, dim3(1), dim3(64), 0, ctx->stream, (const u64 *)q.counters, stats);
    GH_CHECK_HIP(ctx, hipGetLastError());
    return sg.finish();
}

}  // namespace

}  // namespace gridhip

using namespace gridhip;

extern "C" {

int gridhip_contsub(gridhip_ctx *ctx, int64_t R, int64_t C, int layout, int ncomp, int degree, int mode, const double *x,
                    const uint8_t *chan_mask, const double *data, const double *wt, double nsigma, int64_t niter, double *out,
                    double *coeffs, double *rowinfo, uint8_t *codes, double *stats)
{
    return cs_any(ctx, false, R, C, layout, ncomp, degree, mode, x, chan_mask, data, wt, nsigma, niter, out, coeffs, rowinfo,
                  codes, stats);
}

int gridhip_contsub_dev(gridhip_ctx *ctx, int64_t R, int64_t C, int layout, int ncomp, int degree, int mode, const double *x,
                        const uint8_t *chan_mask, const double *data, const double *wt, double nsigma, int64_t niter,
                        double *out, double *coeffs, double *rowinfo, uint8_t *codes, double *stats)
{
    return cs_any(ctx, true, R, C, layout, ncomp, degree, mode, x, chan_mask, data, wt, nsigma, niter, out, coeffs, rowinfo,
                  codes, stats);
}

int gridhip_contsub_tile(int64_t *out)
{
    if (!out) return GRIDHIP_EINVAL;
    out[0] = CS_ROWS, out[1] = CS_CHUNK;
    return GRIDHIP_OK;
}

}  // extern "C"
