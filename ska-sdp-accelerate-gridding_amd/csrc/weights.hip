// Imaging weights (include/gridhip.h, "imaging weights"): natural, uniform and Briggs weighting with a Gaussian uv taper
// and per-visibility data weights, as a device-resident step of its own and as what an imager makes at creation.
//
//     weights_zero_kernel     the density and the two sums over the cells start from zero (a kernel: no memset node)
//     weights_density_kernel  pass 1 over the visibilities: the doweight cell of (u / lam, v / lam), the flag, the density
//                             (uint32 counts without data weights, fp64 global atomics with them); leaves the 8-byte
//                             cell code for pass 2, which then reads neither u nor v again unless there is a taper
//     weights_cellsum_kernel  Briggs only: sum D and sum D^2 over the N^2 cells (64-bit integers for counts: exact and
//                             independent of the schedule)
//     weights_apply_kernel    pass 2: w_k from the cell code, the data weight and the taper, and the six sums of `stats`
//                             in the same pass - one row of partial sums per work-group, no atomics
//     weights_stats_kernel    one work-group adds the rows in a fixed order and writes the 8 doubles
// Natural weighting needs no density: pass 2 takes the cell itself (it is needed for the bookkeeping only) and is the one
// pass over the visibilities.  f^2 lives on the device: pass 2 and the stats kernel derive it from the two sums.
// Both passes are HBM-bound streams.  With stride 1 and 16-byte aligned arrays a lane takes two adjacent visibilities
// with 16-byte loads and stores; any other stride or alignment takes them one by one.
#include "common.h"
#include "imaging.h"

namespace gridhip {

namespace {

constexpr int WT_ACC_HEAD = 8;  // 8-byte words before the partial sums: [0] sum D, [1] sum D^2
constexpr int WT_PARTS = 6;     // sum w, sum w^2 / s, sum s, used, flagged, outside

// the sum of x over the work-group's 256 threads, in a fixed order, in every thread; lds: 4 values
template <typename T>
__device__ __forceinline__ T block_sum(T x, T *lds)
{
    for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o);
    __syncthreads();  // (lds may still be read from the last sum)
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = x;
    __syncthreads();
    return ((lds[0] + lds[1]) + lds[2]) + lds[3];
}

// nq 16-byte units of zeros from a (16-byte aligned), and the head of acc
__global__ void __launch_bounds__(256) weights_zero_kernel(int64_t nq, uint4 *__restrict__ a, unsigned long long *__restrict__ acc)
{
    const int64_t k0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (int64_t k = k0; k < nq; k += (int64_t)gridDim.x * blockDim.x) a[k] = make_uint4(0u, 0u, 0u, 0u);
    if (k0 < WT_ACC_HEAD) acc[k0] = 0ull;
}

// pass 1.  VEC: stride 1, u, v, wt_in (when given) and cell 16-byte aligned
template <bool VEC>
__global__ void __launch_bounds__(256)
    weights_density_kernel(int64_t n, const double *__restrict__ u, const double *__restrict__ v, int64_t stride, double lam,
                           int64_t N, const double *__restrict__ wt_in, int64_t *__restrict__ cell,
                           unsigned int *__restrict__ cnt, double *__restrict__ dens)
{
    const int64_t k0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, step = (int64_t)gridDim.x * blockDim.x;
    if (VEC) {
        const int64_t pairs = n / 2;
        for (int64_t i = k0; i < pairs; i += step) {
            const double2 uu = reinterpret_cast<const double2 *>(u)[i], vv = reinterpret_cast<const double2 *>(v)[i];
            longlong2 c;
            c.x = weight_note(weight_cell(N, uu.x / lam, vv.x / lam), wt_in, 2 * i, cnt, dens);
            c.y = weight_note(weight_cell(N, uu.y / lam, vv.y / lam), wt_in, 2 * i + 1, cnt, dens);
            reinterpret_cast<longlong2 *>(cell)[i] = c;
        }
        if (k0 == 0 && (n & 1))
            cell[n - 1] = weight_note(weight_cell(N, u[n - 1] / lam, v[n - 1] / lam), wt_in, n - 1, cnt, dens);
    } else {
        for (int64_t k = k0; k < n; k += step)
            cell[k] = weight_note(weight_cell(N, u[k * stride] / lam, v[k * stride] / lam), wt_in, k, cnt, dens);
    }
}

// Briggs: acc[0] += sum D, acc[1] += sum D^2 over this work-group's cells.  Counts are summed as 64-bit integers (a count
// is below 2^31, so its square and the sum of the squares stay below 2^62); densities in fp64, the work-groups' sums
// meeting in two fp64 atomics.  quads: cells / 4 (counts) or cells / 2 (densities) 16-byte units; the rest one by one.
__global__ void __launch_bounds__(256)
    weights_cellsum_kernel(int64_t cells, const unsigned int *__restrict__ cnt, const double *__restrict__ dens,
                           unsigned long long *__restrict__ acc)
{
    __shared__ unsigned long long li[4];
    __shared__ double ld[4];
    const int64_t k0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, step = (int64_t)gridDim.x * blockDim.x;
    if (cnt) {
        unsigned long long a = 0, b = 0;
        const int64_t quads = cells / 4;
        for (int64_t i = k0; i < quads; i += step) {
            const uint4 q = reinterpret_cast<const uint4 *>(cnt)[i];
            a += (unsigned long long)q.x + q.y + q.z + q.w;
            b += (unsigned long long)q.x * q.x + (unsigned long long)q.y * q.y + (unsigned long long)q.z * q.z +
                 (unsigned long long)q.w * q.w;
        }
        for (int64_t k = 4 * quads + k0; k < cells; k += step) {
            const unsigned long long c = cnt[k];
            a += c;
            b += c * c;
        }
        a = block_sum(a, li);
        b = block_sum(b, li);
        if (threadIdx.x == 0 && a) {
            atomicAdd(&acc[0], a);
            atomicAdd(&acc[1], b);
        }
    } else {
        double a = 0.0, b = 0.0;
        const int64_t pairs = cells / 2;
        for (int64_t i = k0; i < pairs; i += step) {
            const double2 q = reinterpret_cast<const double2 *>(dens)[i];
            a += q.x + q.y;
            b += q.x * q.x + q.y * q.y;
        }
        for (int64_t k = 2 * pairs + k0; k < cells; k += step) {
            const double c = dens[k];
            a += c;
            b += c * c;
        }
        a = block_sum(a, ld);
        b = block_sum(b, ld);
        if (threadIdx.x == 0 && a != 0.0) {
            atomicAdd(reinterpret_cast<double *>(&acc[0]), a);
            atomicAdd(reinterpret_cast<double *>(&acc[1]), b);
        }
    }
}

// f^2 = b2 / (sum D^2 / sum D), b2 = (5 * 10^-R)^2 from the host; 0 where nothing lies in the grid
__device__ __forceinline__ double briggs_f2(const unsigned long long *acc, bool counts, double b2)
{
    const double sd = counts ? (double)acc[0] : __builtin_bit_cast(double, acc[0]);
    const double sd2 = counts ? (double)acc[1] : __builtin_bit_cast(double, acc[1]);
    return sd > 0.0 ? b2 / (sd2 / sd) : 0.0;
}

struct Sums {
    double w = 0.0, w2s = 0.0, s = 0.0;
    unsigned int used = 0, flagged = 0, outside = 0;  // (a lane sees far fewer than 2^32 visibilities)
};

// What pass 2 needs besides the arrays
struct ApplyArgs {
    int mode;
    bool counts, keep_sign;
    double b2, den;  // Briggs' (5 * 10^-R)^2 ; the taper's 2 sigma^2, 0: no taper
    double lam;
    int64_t N;
};

// one visibility: c its cell code, s its data weight (1 without), r2 = u^2 + v^2 (read only with a taper)
__device__ __forceinline__ double weigh_one(const ApplyArgs &a, int64_t c, double s, double r2, double f2,
                                            const unsigned int *__restrict__ cnt, const double *__restrict__ dens, Sums &sum)
{
#pragma clang fp contract(off)
    if (c == WEIGHT_FLAGGED) {
        ++sum.flagged;
        return 0.0;
    }
    const double t = a.den > 0.0 ? exp(-(r2 / a.den)) : 1.0;
    if (c < 0) {
        ++sum.outside;
        return s * t;
    }
    double w = s;
    if (a.mode == 1) {
        w = s / (a.counts ? (double)cnt[c] : dens[c]);
    } else if (a.mode == 2) {
        const double p = (a.counts ? (double)cnt[c] : dens[c]) * f2;
        w = s / (1.0 + p);
    }
    w = w * t;
    sum.w += w;
    sum.w2s += w * w / s;
    sum.s += s;
    ++sum.used;
    return w;
}

// pass 2.  cell null: the cell is taken here (natural weighting).  out may be wt_in (element k is read before it is
// written, by the same lane): no __restrict__ on either.  VEC as in pass 1, for every array the call reads or writes.
template <bool VEC>
__global__ void __launch_bounds__(256)
    weights_apply_kernel(int64_t n, ApplyArgs a, const int64_t *__restrict__ cell, const double *wt_in,
                         const double *__restrict__ u, const double *__restrict__ v, int64_t stride,
                         const unsigned int *__restrict__ cnt, const double *__restrict__ dens,
                         const unsigned long long *__restrict__ acc, double *out, double *__restrict__ parts)
{
#pragma clang fp contract(off)
    __shared__ double lds[4];
    const int64_t k0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, step = (int64_t)gridDim.x * blockDim.x;
    const double f2 = a.mode == 2 ? briggs_f2(acc, a.counts, a.b2) : 0.0;
    const bool uv = a.den > 0.0 || !cell;
    Sums sum;
    auto code = [&](int64_t k, double u0, double v0) -> int64_t {
        if (cell) return cell[k];
        return weight_note(weight_cell(a.N, u0 / a.lam, v0 / a.lam), wt_in, k, nullptr, nullptr);
    };
    if (VEC) {
        const int64_t pairs = n / 2;
        for (int64_t i = k0; i < pairs; i += step) {
            double2 uu = make_double2(0.0, 0.0), vv = uu, ss = make_double2(1.0, 1.0);
            if (uv) uu = reinterpret_cast<const double2 *>(u)[i], vv = reinterpret_cast<const double2 *>(v)[i];
            if (wt_in) ss = reinterpret_cast<const double2 *>(wt_in)[i];
            longlong2 c;
            if (cell)
                c = reinterpret_cast<const longlong2 *>(cell)[i];
            else
                c.x = code(2 * i, uu.x, vv.x), c.y = code(2 * i + 1, uu.y, vv.y);
            double2 w;
            w.x = weigh_one(a, c.x, ss.x, uu.x * uu.x + vv.x * vv.x, f2, cnt, dens, sum);
            w.y = weigh_one(a, c.y, ss.y, uu.y * uu.y + vv.y * vv.y, f2, cnt, dens, sum);
            if (a.keep_sign) {
                const double2 o = reinterpret_cast<const double2 *>(out)[i];
                w.x = copysign(w.x, o.x), w.y = copysign(w.y, o.y);
            }
            reinterpret_cast<double2 *>(out)[i] = w;
        }
    }
    for (int64_t k = VEC ? (k0 == 0 && (n & 1) ? n - 1 : n) : k0; k < n; k += step) {
        const double u0 = uv ? u[k * stride] : 0.0, v0 = uv ? v[k * stride] : 0.0;
        const double s = wt_in ? wt_in[k] : 1.0;
        double w = weigh_one(a, code(k, u0, v0), s, u0 * u0 + v0 * v0, f2, cnt, dens, sum);
        if (a.keep_sign) w = copysign(w, out[k]);
        out[k] = w;
    }
    const double r[WT_PARTS] = {sum.w, sum.w2s, sum.s, (double)sum.used, (double)sum.flagged, (double)sum.outside};
    for (int j = 0; j < WT_PARTS; ++j) {
        const double x = block_sum(r[j], lds);
        if (threadIdx.x == 0) parts[(int64_t)blockIdx.x * WT_PARTS + j] = x;
    }
}

// stats = { sum w, sum w^2 / s, sum s, noise, f^2, used, flagged, outside } from nblk rows of partial sums: thread t adds
// the rows t, t + 256, ... in order, the 256 sums meet in block_sum's fixed order
__global__ void __launch_bounds__(256)
    weights_stats_kernel(int nblk, const double *__restrict__ parts, const unsigned long long *__restrict__ acc, int mode,
                         bool counts, double b2, double *__restrict__ stats)
{
    __shared__ double lds[4];
    double tot[WT_PARTS];
    for (int j = 0; j < WT_PARTS; ++j) {
        double x = 0.0;
        for (int b = threadIdx.x; b < nblk; b += 256) x += parts[(int64_t)b * WT_PARTS + j];
        tot[j] = block_sum(x, lds);
    }
    if (threadIdx.x != 0) return;
    stats[0] = tot[0];
    stats[1] = tot[1];
    stats[2] = tot[2];
    stats[3] = tot[0] != 0.0 ? sqrt(tot[1] * tot[2]) / tot[0] : __builtin_nan("");
    stats[4] = mode == 2 ? briggs_f2(acc, counts, b2) : 0.0;
    stats[5] = tot[3];
    stats[6] = tot[4];
    stats[7] = tot[5];
}

bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

int weights_mode_check(gridhip_ctx *ctx, int mode, double robust, double sigma)
{
    if (mode < 0 || mode > 2 || !(robust - robust == 0.0) || !(sigma >= 0.0))
        return fail(ctx, GRIDHIP_EINVAL, "weights: mode 0..2, a finite robust and taper_sigma >= 0");
    return GRIDHIP_OK;
}

int weights_begin(gridhip_ctx *ctx, int64_t N, int mode, bool data_weights, WeightScratch &s)
{
    const size_t cells = (size_t)N * N;
    const size_t dbytes = mode == 0 ? 0 : ((cells * (data_weights ? 8 : 4) + 15) / 16) * 16;
    GH_CHECK(s.dens.alloc(ctx, dbytes));
    GH_CHECK(s.acc.alloc(ctx, (WT_ACC_HEAD + (size_t)WT_PARTS * ctx->num_cu * 16) * 8));
    s.cnt = mode != 0 && !data_weights ? s.dens.as<unsigned int>() : nullptr;
    s.den = mode != 0 && data_weights ? s.dens.as<double>() : nullptr;
    hipLaunchKernelGGL(weights_zero_kernel, grid_for(ctx, (int64_t)(dbytes / 16)), dim3(256), 0, ctx->stream,
                       (int64_t)(dbytes / 16), s.dens.as<uint4>(), s.acc.as<unsigned long long>());
    GH_CHECK_HIP(ctx, hipGetLastError());
    return GRIDHIP_OK;
}

int weights_finish(gridhip_ctx *ctx, int64_t N, int64_t n, int mode, double robust, double sigma, const int64_t *cell,
                   WeightScratch &s, const double *wt_in, const double *u, const double *v, int64_t stride, double lam,
                   double *out, bool keep_sign, double *stats)
{
    const double b = 5.0 * pow(10.0, -robust);
    ApplyArgs a{mode, wt_in == nullptr, keep_sign, b * b, 2.0 * sigma * sigma, lam, N};
    unsigned long long *acc = s.acc.as<unsigned long long>();
    double *parts = s.acc.as<double>() + WT_ACC_HEAD;
    if (mode == 2)
        hipLaunchKernelGGL(weights_cellsum_kernel, grid_for(ctx, N * N / 4), dim3(256), 0, ctx->stream, N * N, s.cnt, s.den,
                           acc);
    int nblk = 0;
    if (n > 0) {
        const bool uv = a.den > 0.0 || !cell;
        const bool vec = stride == 1 && aligned16(out) && aligned16(wt_in) && aligned16(cell) &&
                         (!uv || (aligned16(u) && aligned16(v)));
        const dim3 grid = grid_for(ctx, vec ? (n + 1) / 2 : n);
        nblk = (int)grid.x;
        if (vec)
            hipLaunchKernelGGL(weights_apply_kernel<true>, grid, dim3(256), 0, ctx->stream, n, a, cell, wt_in, u, v, stride,
                               s.cnt, s.den, acc, out, parts);
        else
            hipLaunchKernelGGL(weights_apply_kernel<false>, grid, dim3(256), 0, ctx->stream, n, a, cell, wt_in, u, v, stride,
                               s.cnt, s.den, acc, out, parts);
    }
    if (stats)
        hipLaunchKernelGGL(weights_stats_kernel, dim3(1), dim3(256), 0, ctx->stream, nblk, parts, acc, mode, a.counts, a.b2,
                           stats);
    GH_CHECK_HIP(ctx, hipGetLastError());
    return GRIDHIP_OK;
}

}  // namespace gridhip

using namespace gridhip;

namespace {

// gridhip_weights' argument rules; *N = the image size
int weights_check(gridhip_ctx *ctx, double theta, int64_t lam, int64_t n, const double *u, const double *v, int64_t stride,
                  int mode, double robust, double sigma, const double *wt_out, int64_t *N)
{
    *N = gridhip_image_size(theta, lam);
    if (*N < 1 || n < 0 || stride < 1 || (n > 0 && (!u || !v || !wt_out)))
        return fail(ctx, GRIDHIP_EINVAL, "weights: bad argument");
    GH_CHECK(weights_mode_check(ctx, mode, robust, sigma));
    if (overlaps_any({wt_out, (size_t)n * 8}, {{u, span_bytes(n, stride)}, {v, span_bytes(n, stride)}}))
        return fail(ctx, GRIDHIP_EINVAL, "weights: wt_out may be wt_in itself, and overlap neither u nor v");
    return GRIDHIP_OK;
}

// the device form on checked arguments: kernels only, on ctx->stream
int weights_run(gridhip_ctx *ctx, int64_t N, double lam, int64_t n, const double *u, const double *v, int64_t stride,
                const double *wt_in, int mode, double robust, double sigma, double *wt_out, double *stats)
{
    WeightScratch s;
    DevBuf cell;
    GH_CHECK(weights_begin(ctx, N, mode, wt_in != nullptr, s));
    if (mode != 0 && n > 0) {
        GH_CHECK(cell.alloc(ctx, (size_t)n * 8));
        const bool vec = stride == 1 && ((uintptr_t)u & 15) == 0 && ((uintptr_t)v & 15) == 0 && ((uintptr_t)wt_in & 15) == 0;
        const dim3 grid = grid_for(ctx, vec ? (n + 1) / 2 : n);
        if (vec)
            hipLaunchKernelGGL(weights_density_kernel<true>, grid, dim3(256), 0, ctx->stream, n, u, v, stride, lam, N, wt_in,
                               cell.as<int64_t>(), s.cnt, s.den);
        else
            hipLaunchKernelGGL(weights_density_kernel<false>, grid, dim3(256), 0, ctx->stream, n, u, v, stride, lam, N,
                               wt_in, cell.as<int64_t>(), s.cnt, s.den);
        GH_CHECK_HIP(ctx, hipGetLastError());
    }
    return weights_finish(ctx, N, n, mode, robust, sigma, cell.as<int64_t>(), s, wt_in, u, v, stride, lam, wt_out, false,
                          stats);
}

int weights_any(gridhip_ctx *ctx, bool dev, double theta, int64_t lam, int64_t n, const double *u, const double *v,
                int64_t uv_stride, const double *wt_in, int mode, double robust, double taper_sigma, double *wt_out,
                double *stats)
{
    if (!ctx) return GRIDHIP_EINVAL;
    int64_t N = 0;
    GH_CHECK(weights_check(ctx, theta, lam, n, u, v, uv_stride, mode, robust, taper_sigma, wt_out, &N));
    GH_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    Staged st(ctx, dev);
    u = st.in(u, span_bytes(n, uv_stride)), v = st.in(v, span_bytes(n, uv_stride)), wt_in = st.in(wt_in, (size_t)n * 8);
    wt_out = st.out(wt_out, (size_t)n * 8), stats = st.out(stats, 64);
    GH_CHECK(st.status());
    GH_CHECK(weights_run(ctx, N, (double)lam, n, u, v, uv_stride, wt_in, mode, robust, taper_sigma, wt_out, stats));
    return st.finish();
}

}  // namespace

extern "C" {

int gridhip_weights_dev(gridhip_ctx *ctx, double theta, int64_t lam, int64_t n, const double *u, const double *v,
                        int64_t uv_stride, const double *wt_in, int mode, double robust, double taper_sigma, double *wt_out,
                        double *stats)
{
    return weights_any(ctx, true, theta, lam, n, u, v, uv_stride, wt_in, mode, robust, taper_sigma, wt_out, stats);
}

int gridhip_weights(gridhip_ctx *ctx, double theta, int64_t lam, int64_t n, const double *u, const double *v,
                    int64_t uv_stride, const double *wt_in, int mode, double robust, double taper_sigma, double *wt_out,
                    double *stats)
{
    return weights_any(ctx, false, theta, lam, n, u, v, uv_stride, wt_in, mode, robust, taper_sigma, wt_out, stats);
}

}  // extern "C"
