// Reprojection and mosaicking (include/gridhip.h, "reprojection and mosaicking"): F images on F tangent planes, each a
// rotation away from the destination plane, resampled onto that plane and combined into one weighted, feathered image.
//
// One gridhip_mosaic call is two launches, three with stats:
//     mosaic_prologue_kernel  one work-group: R_f of every facet judged by phase_shift's rule (finite, R22 > 0, orthonormal
//                             to 1e-9) and copied with its verdict into the scratch block; the counters of the call are
//                             written here (plain stores: no memset node)
//     mosaic_kernel<KIND>     one thread per destination cell, 16 x 16 cells per work-group.  The work-group first culls:
//                             the facets that can reach its tile go, in ascending order, into a list in LDS, and the
//                             threads then walk that list - the order of the list is the order of the sums, so the cull
//                             changes no bit.  Every lane owns its cell's num and den: no atomic on a double anywhere.
//     mosaic_stats_kernel     the 8 doubles
// THE CULL'S BOUND.  The map from the destination plane to a facet's plane is not affine - n = sqrt(1 - l^2 - m^2) enters
// it - so a tile is not bounded by its corners.  It is bounded in three dimensions instead: every cell of the tile has
// l in [l(x0), l(x1)], m in [m(y0), m(y1)] and n in [sqrt(1 - r2max), sqrt(1 - r2min)], r2min and r2max taken at the
// point of the rectangle nearest to and farthest from the origin, and (l', m', n') = R (l, m, n) IS linear on that box:
// the interval sum of the three products bounds it.  Every operation of the cell rule - a rounded product with a constant,
// a rounded sum, x * x for x >= 0, sqrt, the division by theta, |fx - Ns/2| on either side - is monotone, and the bound is
// formed with the same operations in the same order, so it holds for the rounded values, not just for the exact ones:
// no margin is needed.  A facet stays on the list unless the box proves n' <= 0 everywhere, or fx (fy) beyond the window
// (|fx - Ns/2| > outer) or beyond the taps ([-1, Ns]) everywhere.  The box is wider than the patch of the sphere it holds,
// most of all near the horizon: the list is a superset, and the cell rule decides.
// Integer atomics only (the counters, one per wave); contraction is off for the whole file.
#include <math.h>

#include "common.h"
#include "imaging.h"

#pragma clang fp contract(off)

namespace gridhip {

namespace {

typedef unsigned long long u64;
typedef unsigned int u32;

constexpr int64_t MOSAIC_MAX_F = 4096;   // the LDS list holds 16-bit facet indices
constexpr int64_t MOSAIC_MAX_N = 32768;
constexpr int MOSAIC_TILE = 16;

struct FacetInfo {  // 80 bytes per facet in the scratch block
    double r[9];
    int valid, pad;
};

struct MosaicCounts {  // 256 bytes at the head of the scratch block
    u64 covered, left;  // destination cells with den > wmin; samples left out for a tap that is not finite
    u32 used, refused, most, pad0;
    u64 pad[28];
};
static_assert(sizeof(MosaicCounts) == 256, "the counter block");

struct MosaicArgs {
    int F, Ns, Nd, normalize, cull, count;
    double theta_s, theta_d, inner, outer, wmin, blank;
    const double *facets, *weights;
    double *out, *wsum;
    const FacetInfo *info;
    MosaicCounts *counts;
};

__device__ __forceinline__ bool is_fin(double x) { return x - x == 0.0; }

// phase_shift's rule for one R (average.hip, rotation_check), on the device
__device__ __forceinline__ bool rotation_ok(const double *R)
{
    bool ok = true;
    for (int i = 0; i < 9; ++i) ok = ok && is_fin(R[i]);
    ok = ok && R[8] > 0.0;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const double d = R[3 * i] * R[3 * j] + R[3 * i + 1] * R[3 * j + 1] + R[3 * i + 2] * R[3 * j + 2] - (i == j ? 1.0 : 0.0);
            ok = ok && fabs(d) <= 1e-9;
        }
    return ok;
}

__global__ void __launch_bounds__(256) mosaic_prologue_kernel(int F, const double *__restrict__ R, FacetInfo *__restrict__ info,
                                                              MosaicCounts *__restrict__ counts)
{
    __shared__ u32 good[256];
    u32 mine = 0u;
    for (int f = threadIdx.x; f < F; f += 256) {
        double r[9];
        for (int i = 0; i < 9; ++i) r[i] = R[(int64_t)f * 9 + i];
        const bool ok = rotation_ok(r);
        for (int i = 0; i < 9; ++i) info[f].r[i] = r[i];
        info[f].valid = ok ? 1 : 0;
        info[f].pad = 0;
        mine += ok ? 1u : 0u;
    }
    good[threadIdx.x] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        u32 all = 0u;
        for (int t = 0; t < 256; ++t) all += good[t];
        counts->covered = 0ull;
        counts->left = 0ull;
        counts->used = all;
        counts->refused = (u32)F - all;
        counts->most = 0u;
    }
}

// the feather of one axis: 1 inside `inner`, 0 from `outer` on, the smoothstep between
__device__ __forceinline__ double feather(double d, double inner, double outer)
{
    if (d <= inner) return 1.0;
    if (d >= outer) return 0.0;
    const double t = (outer - d) / (outer - inner);
    return (t * t) * (3.0 - 2.0 * t);
}

// Keys' cubic convolution, a = -1/2, in Horner form
__device__ __forceinline__ void keys(double t, double c[4])
{
    c[0] = ((-0.5 * t + 1.0) * t - 0.5) * t;
    c[1] = ((1.5 * t - 2.5) * t) * t + 1.0;
    c[2] = ((-1.5 * t + 2.0) * t + 0.5) * t;
    c[3] = ((0.5 * t - 0.5) * t) * t;
}

// the bilinear sample of the Ns x Ns image p at (fx, fy); false: a tap of its footprint lies outside the image
__device__ __forceinline__ bool bilinear(const double *__restrict__ p, int Ns, double fx, double fy, double *v, bool *fin)
{
    const double ix = floor(fx), iy = floor(fy);
    if (!(ix >= 0.0 && ix <= (double)(Ns - 2) && iy >= 0.0 && iy <= (double)(Ns - 2))) return false;
    const double tx = fx - ix, ty = fy - iy;
    const double *q = p + (int64_t)iy * Ns + (int64_t)ix;
    const double a = q[0], b = q[1], c = q[Ns], d = q[(int64_t)Ns + 1];
    *fin = is_fin(a) && is_fin(b) && is_fin(c) && is_fin(d);
    const double r0 = a * (1.0 - tx) + b * tx, r1 = c * (1.0 - tx) + d * tx;
    *v = r0 * (1.0 - ty) + r1 * ty;
    return true;
}

template <int KIND>
__device__ __forceinline__ bool sample(const double *__restrict__ p, int Ns, double fx, double fy, double *v, bool *fin)
{
    if (KIND == 0) {
        const double cx = floor(0.5 + fx), cy = floor(0.5 + fy);
        if (!(cx >= 0.0 && cx <= (double)(Ns - 1) && cy >= 0.0 && cy <= (double)(Ns - 1))) return false;
        *v = p[(int64_t)cy * Ns + (int64_t)cx];
        *fin = is_fin(*v);
        return true;
    }
    if (KIND == 1) return bilinear(p, Ns, fx, fy, v, fin);
    const double ix = floor(fx), iy = floor(fy);
    if (!(ix >= 1.0 && ix <= (double)(Ns - 3) && iy >= 1.0 && iy <= (double)(Ns - 3))) return false;
    double cx[4], cy[4], row[4];
    keys(fx - ix, cx);
    keys(fy - iy, cy);
    const double *q = p + ((int64_t)iy - 1) * Ns + ((int64_t)ix - 1);
    bool f = true;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const double a = q[0], b = q[1], c = q[2], d = q[3];
        f = f && is_fin(a) && is_fin(b) && is_fin(c) && is_fin(d);
        row[j] = ((cx[0] * a + cx[1] * b) + cx[2] * c) + cx[3] * d;
        q += Ns;
    }
    *fin = f;
    *v = ((cy[0] * row[0] + cy[1] * row[1]) + cy[2] * row[2]) + cy[3] * row[3];
    return true;
}

// the interval of (a x + b y) + c z over x in [x0, x1], y in [y0, y1], z in [z0, z1], with the cell rule's own roundings
__device__ __forceinline__ void row_bounds(double a, double b, double c, double x0, double x1, double y0, double y1, double z0,
                                           double z1, double *lo, double *hi)
{
    const double ax0 = a * x0, ax1 = a * x1, by0 = b * y0, by1 = b * y1, cz0 = c * z0, cz1 = c * z1;
    *lo = (fmin(ax0, ax1) + fmin(by0, by1)) + fmin(cz0, cz1);
    *hi = (fmax(ax0, ax1) + fmax(by0, by1)) + fmax(cz0, cz1);
}

// can a coordinate whose l' (m') lies in [lo, hi] pass the window and the taps?
__device__ __forceinline__ bool axis_reaches(double lo, double hi, int Ns, double theta_s, double outer)
{
    const double h = (double)(Ns / 2);
    const double flo = (lo * (double)Ns) / theta_s + h, fhi = (hi * (double)Ns) / theta_s + h;
    if (flo - h > outer || h - fhi > outer) return false;  // |fx - Ns/2| > outer for every cell
    if (fhi < -1.0 || flo > (double)Ns) return false;      // no tap of any footprint inside
    return true;
}

__device__ __forceinline__ double cell_coord(double theta, int x, int N) { return theta * (double)(x - N / 2) / (double)N; }

template <int KIND>
__global__ void __launch_bounds__(256) mosaic_kernel(MosaicArgs a)
{
    __shared__ unsigned short list[MOSAIC_MAX_F];
    __shared__ u32 rank_lds[4];
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * MOSAIC_TILE, y0 = blockIdx.y * MOSAIC_TILE;
    const int x = x0 + (tid & (MOSAIC_TILE - 1)), y = y0 + (tid >> 4);

    // ---- the cull: the tile's box in (l, m, n) ----
    const int x1 = min(x0 + MOSAIC_TILE - 1, a.Nd - 1), y1 = min(y0 + MOSAIC_TILE - 1, a.Nd - 1);
    const double bl0 = cell_coord(a.theta_d, x0, a.Nd), bl1 = cell_coord(a.theta_d, x1, a.Nd);
    const double bm0 = cell_coord(a.theta_d, y0, a.Nd), bm1 = cell_coord(a.theta_d, y1, a.Nd);
    const double lnear = (bl0 <= 0.0 && bl1 >= 0.0) ? 0.0 : fmin(fabs(bl0), fabs(bl1)), lfar = fmax(fabs(bl0), fabs(bl1));
    const double mnear = (bm0 <= 0.0 && bm1 >= 0.0) ? 0.0 : fmin(fabs(bm0), fabs(bm1)), mfar = fmax(fabs(bm0), fabs(bm1));
    const double r2min = lnear * lnear + mnear * mnear, r2max = lfar * lfar + mfar * mfar;
    const bool tile_live = r2min < 1.0;  // (else every cell of the tile lies beyond the horizon)
    const double bn1 = tile_live ? sqrt(1.0 - r2min) : 0.0, bn0 = r2max < 1.0 ? sqrt(1.0 - r2max) : 0.0;
    int nlist = 0;
    for (int base = 0; base < a.F; base += 256) {
        const int f = base + tid;
        bool keep = false;
        if (f < a.F && tile_live && a.info[f].valid) {
            keep = true;
            if (a.cull) {
                const double *r = a.info[f].r;
                double lo, hi;
                row_bounds(r[6], r[7], r[8], bl0, bl1, bm0, bm1, bn0, bn1, &lo, &hi);
                keep = !(hi <= 0.0);  // (n' > 0 somewhere; a bound that is not a number decides nothing)
                if (keep) {
                    row_bounds(r[0], r[1], r[2], bl0, bl1, bm0, bm1, bn0, bn1, &lo, &hi);
                    keep = axis_reaches(lo, hi, a.Ns, a.theta_s, a.outer);
                }
                if (keep) {
                    row_bounds(r[3], r[4], r[5], bl0, bl1, bm0, bm1, bn0, bn1, &lo, &hi);
                    keep = axis_reaches(lo, hi, a.Ns, a.theta_s, a.outer);
                }
            }
        }
        u32 total;
        const u32 before = block_rank(keep ? 1u : 0u, rank_lds, &total);
        if (keep) list[nlist + (int)before] = (unsigned short)f;
        nlist += (int)total;
    }
    __syncthreads();

    // ---- the cell ----
    const bool inside = x < a.Nd && y < a.Nd;
    const double l = cell_coord(a.theta_d, x, a.Nd), m = cell_coord(a.theta_d, y, a.Nd);
    const double r2 = l * l + m * m;
    const bool live = inside && r2 < 1.0;
    const double n = live ? sqrt(1.0 - r2) : 0.0;
    const double h = (double)(a.Ns / 2);
    const int64_t plane = (int64_t)a.Ns * a.Ns;
    double num = 0.0, den = 0.0;
    u32 cnt = 0u, left = 0u;
    if (live) {
        for (int j = 0; j < nlist; ++j) {
            const int f = __builtin_amdgcn_readfirstlane((int)list[j]);  // (the same for every lane: scalar loads of R_f)
            const double *r = a.info[f].r;
            const double np = (r[6] * l + r[7] * m) + r[8] * n;
            if (!(np > 0.0)) continue;
            const double lp = (r[0] * l + r[1] * m) + r[2] * n, mp = (r[3] * l + r[4] * m) + r[5] * n;
            const double fx = (lp * (double)a.Ns) / a.theta_s + h, fy = (mp * (double)a.Ns) / a.theta_s + h;
            double w = feather(fabs(fx - h), a.inner, a.outer) * feather(fabs(fy - h), a.inner, a.outer);
            if (w == 0.0) continue;
            double v;
            bool fin;
            if (!sample<KIND>(a.facets + (int64_t)f * plane, a.Ns, fx, fy, &v, &fin)) continue;
            if (!fin) {
                left += 1u;
                continue;
            }
            if (a.weights) {
                double q;
                bool qfin;
                if (!bilinear(a.weights + (int64_t)f * plane, a.Ns, fx, fy, &q, &qfin)) continue;
                (void)qfin;  // (q itself is judged: a tap that is not finite makes it so)
                if (!(is_fin(q) && q > 0.0)) continue;
                w = w * q;
            }
            num = num + w * v;
            den = den + w;
            cnt += 1u;
        }
    }
    const bool covered = live && den > a.wmin;
    if (inside) {
        const int64_t c = (int64_t)y * a.Nd + x;
        a.out[c] = covered ? (a.normalize ? num / den : num) : a.blank;
        if (a.wsum) a.wsum[c] = covered ? den : 0.0;
    }
    if (a.count) {
        u32 cov = covered ? 1u : 0u;
        for (int o = 32; o > 0; o >>= 1) {
            cov += __shfl_down(cov, o);
            left += __shfl_down(left, o);
            const u32 t = __shfl_down(cnt, o);
            cnt = t > cnt ? t : cnt;
        }
        if ((tid & 63) == 0) {
            if (cov) atomicAdd(&a.counts->covered, (u64)cov);
            if (left) atomicAdd(&a.counts->left, (u64)left);
            if (cnt) atomicMax(&a.counts->most, cnt);
        }
    }
}

__global__ void __launch_bounds__(64) mosaic_stats_kernel(int64_t cells, const MosaicCounts *counts, double *__restrict__ stats)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    stats[0] = (double)counts->covered;
    stats[1] = (double)((u64)cells - counts->covered);
    stats[2] = (double)counts->used;
    stats[3] = (double)counts->refused;
    stats[4] = (double)counts->left;
    stats[5] = (double)counts->most;
    stats[6] = 0.0;
    stats[7] = 0.0;
}

}  // namespace

int mosaic_check(gridhip_ctx *ctx, int64_t F, int64_t Ns, double theta_s, const double *facets, const double *weights,
                 const double *R, int kind, double inner, double outer, double wmin, int64_t Nd, double theta_d,
                 const double *out, const double *wsum, const double *stats)
{
    if (!facets || !R || !out || F < 1 || Ns < 1 || Nd < 1)
        return fail(ctx, GRIDHIP_EINVAL, "mosaic: facets, R and out, F >= 1, Ns >= 1, Nd >= 1");
    if (!(std::isfinite(theta_s) && theta_s > 0.0 && std::isfinite(theta_d) && theta_d > 0.0))
        return fail(ctx, GRIDHIP_EINVAL, "mosaic: theta_s and theta_d must be finite and > 0");
    if (kind != 0 && kind != 1 && kind != 3)
        return fail(ctx, GRIDHIP_EINVAL, "mosaic: kind must be 0 (nearest), 1 (bilinear) or 3 (cubic)");
    if (!(std::isfinite(inner) && std::isfinite(outer) && inner >= 0.0 && outer >= inner))
        return fail(ctx, GRIDHIP_EINVAL, "mosaic: the window needs finite 0 <= inner <= outer");
    if (!(wmin >= 0.0)) return fail(ctx, GRIDHIP_EINVAL, "mosaic: wmin must be >= 0");
    if (F <= MOSAIC_MAX_F && Ns <= MOSAIC_MAX_N && Nd <= MOSAIC_MAX_N) {  // (sizes that overflow nothing)
        const size_t fb = (size_t)F * (size_t)Ns * (size_t)Ns * 8, ob = (size_t)Nd * (size_t)Nd * 8;
        const int clash = outputs_clash({{out, ob}, {wsum, ob}, {stats, 64}}, {{facets, fb}, {weights, fb}, {R, (size_t)F * 72}});
        if (clash == 1) return fail(ctx, GRIDHIP_EINVAL, "mosaic: an output overlaps an input");
        if (clash == 2) return fail(ctx, GRIDHIP_EINVAL, "mosaic: two outputs overlap");
    }
    if (F > MOSAIC_MAX_F) return fail(ctx, GRIDHIP_EUNSUPPORTED, "mosaic: F must be <= 4096");
    if (Ns > MOSAIC_MAX_N || Nd > MOSAIC_MAX_N) return fail(ctx, GRIDHIP_EUNSUPPORTED, "mosaic: Ns and Nd must be <= 32768");
    return GRIDHIP_OK;
}

size_t mosaic_scratch_bytes(int64_t F) { return sizeof(MosaicCounts) + (size_t)F * sizeof(FacetInfo); }

int mosaic_run(gridhip_ctx *ctx, int64_t F, int64_t Ns, double theta_s, const double *facets, const double *weights,
               const double *R, int kind, double inner, double outer, int normalize, double wmin, double blank, int64_t Nd,
               double theta_d, double *out, double *wsum, double *stats, void *scratch)
{
    MosaicCounts *counts = reinterpret_cast<MosaicCounts *>(scratch);
    FacetInfo *info = reinterpret_cast<FacetInfo *>(reinterpret_cast<char *>(scratch) + sizeof(MosaicCounts));
    hipLaunchKernelGGL(mosaic_prologue_kernel, dim3(1), dim3(256), 0, ctx->stream, (int)F, R, info, counts);
    MosaicArgs a;
    a.F = (int)F, a.Ns = (int)Ns, a.Nd = (int)Nd, a.normalize = normalize ? 1 : 0;
    a.cull = ctx->img->mosaic_cull == 1 ? 0 : 1, a.count = stats ? 1 : 0;
    a.theta_s = theta_s, a.theta_d = theta_d, a.inner = inner, a.outer = outer, a.wmin = wmin, a.blank = blank;
    a.facets = facets, a.weights = weights, a.out = out, a.wsum = wsum, a.info = info, a.counts = counts;
    const unsigned tiles = (unsigned)((Nd + MOSAIC_TILE - 1) / MOSAIC_TILE);
    const dim3 grid(tiles, tiles);
    if (kind == 0)
        hipLaunchKernelGGL(mosaic_kernel<0>, grid, dim3(256), 0, ctx->stream, a);
    else if (kind == 1)
        hipLaunchKernelGGL(mosaic_kernel<1>, grid, dim3(256), 0, ctx->stream, a);
    else
        hipLaunchKernelGGL(mosaic_kernel<3>, grid, dim3(256), 0, ctx->stream, a);
    if (stats) hipLaunchKernelGGL(mosaic_stats_kernel, dim3(1), dim3(64), 0, ctx->stream, Nd * Nd, (const MosaicCounts *)counts, stats);
    GH_CHECK_HIP(ctx, hipGetLastError());
    return GRIDHIP_OK;
}

}  // namespace gridhip

using namespace gridhip;

namespace {

int mosaic_any(gridhip_ctx *ctx, bool dev, int64_t F, int64_t Ns, double theta_s, const double *facets, const double *weights,
               const double *R, int kind, double inner, double outer, int normalize, double wmin, double blank, int64_t Nd,
               double theta_d, double *out, double *wsum, double *stats)
{
    if (!ctx) return GRIDHIP_EINVAL;
    GH_CHECK(mosaic_check(ctx, F, Ns, theta_s, facets, weights, R, kind, inner, outer, wmin, Nd, theta_d, out, wsum, stats));
    GH_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    const size_t fb = (size_t)F * (size_t)Ns * (size_t)Ns * 8, ob = (size_t)Nd * (size_t)Nd * 8;
    DevBuf scratch;
    GH_CHECK(scratch.alloc(ctx, mosaic_scratch_bytes(F)));
    Staged st(ctx, dev);
    facets = st.in(facets, fb), weights = st.in(weights, fb), R = st.in(R, (size_t)F * 72);
    double *dout = st.out(out, ob), *dws = st.out(wsum, ob), *dst = st.out(stats, 64);
    GH_CHECK(st.status());
    GH_CHECK(mosaic_run(ctx, F, Ns, theta_s, facets, weights, R, kind, inner, outer, normalize, wmin, blank, Nd, theta_d, dout,
                        dws, dst, scratch.p));
    return st.finish();
}

}  // namespace

extern "C" {

int gridhip_mosaic_dev(gridhip_ctx *ctx, int64_t F, int64_t Ns, double theta_s, const double *facets, const double *weights,
                       const double *R, int kind, double inner, double outer, int normalize, double wmin, double blank,
                       int64_t Nd, double theta_d, double *out, double *wsum, double *stats)
{
    return mosaic_any(ctx, true, F, Ns, theta_s, facets, weights, R, kind, inner, outer, normalize, wmin, blank, Nd, theta_d, out,
                      wsum, stats);
}

int gridhip_mosaic(gridhip_ctx *ctx, int64_t F, int64_t Ns, double theta_s, const double *facets, const double *weights,
                   const double *R, int kind, double inner, double outer, int normalize, double wmin, double blank, int64_t Nd,
                   double theta_d, double *out, double *wsum, double *stats)
{
    return mosaic_any(ctx, false, F, Ns, theta_s, facets, weights, R, kind, inner, outer, normalize, wmin, blank, Nd, theta_d, out,
                      wsum, stats);
}

int gridhip_reproject_dev(gridhip_ctx *ctx, int64_t Ns, double theta_s, const double *image, const double *R, int kind,
                          double inner, double outer, double blank, int64_t Nd, double theta_d, double *out)
{
    return mosaic_any(ctx, true, 1, Ns, theta_s, image, nullptr, R, kind, inner, outer, 1, 0.0, blank, Nd, theta_d, out, nullptr,
                      nullptr);
}

int gridhip_reproject(gridhip_ctx *ctx, int64_t Ns, double theta_s, const double *image, const double *R, int kind,
                      double inner, double outer, double blank, int64_t Nd, double theta_d, double *out)
{
    return mosaic_any(ctx, false, 1, Ns, theta_s, image, nullptr, R, kind, inner, outer, 1, 0.0, blank, Nd, theta_d, out, nullptr,
                      nullptr);
}

}  // extern "C"
