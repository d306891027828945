// Direct-Fourier prediction of a sky-model component list (include/gridhip.h, "direct-Fourier prediction"):
//     V(u,v,w) = sum_c S_c(x) E_c(u,v) exp(-2 pi i (u l_c + v m_c + w (n_c - 1)))
// exactly - no grid, no kernel truncation, no atomics - and the ordered compaction that turns a model image into such a
// list.  n * C fp64 sine / cosine pairs: the kernel is bound by the fp64 pipe, not by memory.
//
//     dft_prepare_kernel   validates the components and converts each to DFT_PREP doubles { l, m, n - 1, f0 .. f3, quu, quv,
//                          qvv } (E = exp(-(quu u^2 + quv u v + qvv v^2)); all three 0: a point); a skipped component gets
//                          flux 0 and point shape.  One row of { skipped } per work-group, no atomics; thread 0 of
//                          work-group 0 leaves the number of components in use, min(max(*count_dev, 0), C).
//     dft_main_kernel      grid.x over the visibilities, grid.y over the S component slices.  A work-group of 256 threads
//                          takes DFT_WG_VIS = 512 visibilities, each thread the two k0 = base + tid and k0 + 256 (coalesced),
//                          so that two independent sine / cosine chains are in flight per lane.  u, v, w, x and the two
//                          complex accumulators stay in registers.  The work-group stages its slice's prepared components
//                          through LDS in chunks of DFT_CHUNK = 256 (20 KB, so that registers, not LDS, set the residency); the loop
//                          over a chunk is wave-uniform, so every lane reads the same LDS words (a broadcast, no bank
//                          conflict) and the point / Gaussian branch is wave-uniform too.  The phase is formed in turns,
//                          p = u l + v m + w (n - 1), reduced exactly to r = p - rint(p), |r| <= 1/2, and sincospi(2 r)
//                          never needs a large-argument path.  fp64 throughout; no MFMA.
//                          S == 1: the kernel writes vis_out itself (vis_sub - pred in the residual form; element k is
//                          read before it is written, by the same lane).  S > 1: partial sums to part[S][n].
//     dft_epilogue_kernel  S > 1: adds the S partial sums of a visibility in slice order and applies vis_sub.
//     dft_stats_kernel     one work-group adds the rows in a fixed order and writes the 4 doubles.
// Determinism: a visibility's sum runs over the components of a slice in list order in one lane, and over the slices in
// slice order; S depends on (n, C) and the option "dft_slices" only: the same bits on every run.
//
//     cfi_count_kernel, cfi_scan_kernel, cfi_scatter_kernel   gridhip_components_from_image: the non-zero cells of
//                          segments of CFI_SEG = 1024 cells are counted, one work-group scans the counts (exclusive), and
//                          the scatter recounts its segment, orders its cells by a scan over the work-group and writes
//                          row offset + rank while that is below max_c.  Row-major order, the same list on every run.
#include "common.h"
#include "imaging.h"

namespace gridhip {

namespace {

constexpr int DFT_BLOCK = 256;
constexpr int DFT_WG_VIS = 2 * DFT_BLOCK;  // the visibilities of a work-group: two per thread
constexpr int DFT_CHUNK = 256;             // prepared components staged in LDS at a time: 256 * 80 B = 20 KB
constexpr int DFT_PREP = 10;               // doubles of a prepared component
constexpr int DFT_MAX_SLICES = 64;
constexpr int DFT_FILL = 512;              // work-groups that fill the chip (2 per CU of 256): below it, slices
static_assert(DFT_PREP == GRIDHIP_COMP_DOUBLES, "a prepared component takes the room of a given one");

__device__ __forceinline__ bool is_fin(double x) { return x - x == 0.0; }

// the sum of x over the 256 threads of a work-group, in a fixed order, in every thread; lds: 4 values
__device__ __forceinline__ double block_sum256(double x, double *lds)
{
    for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = x;
    __syncthreads();
    return lds[0] + lds[1] + lds[2] + lds[3];
}

__device__ __forceinline__ int64_t comps_in_use(int64_t C, const int64_t *count_dev)
{
    if (!count_dev) return C;
    const int64_t c = *count_dev;
    return c < 0 ? 0 : (c > C ? C : c);
}

// head[0] = components in use; skipped[b] = the skipped ones of work-group b's components
__global__ void __launch_bounds__(DFT_BLOCK)
    dft_prepare_kernel(int64_t C, const double *__restrict__ comps, const int64_t *__restrict__ count_dev, int T,
                       double *__restrict__ prep, int64_t *__restrict__ head, double *__restrict__ skipped)
{
#pragma clang fp contract(off)
    __shared__ double lds[4];
    const int64_t use = comps_in_use(C, count_dev);
    if (blockIdx.x == 0 && threadIdx.x == 0) head[0] = use;
    double skip = 0.0;
    for (int64_t c = (int64_t)blockIdx.x * DFT_BLOCK + threadIdx.x; c < use; c += (int64_t)gridDim.x * DFT_BLOCK) {
        const double *in = comps + c * GRIDHIP_COMP_DOUBLES;
        const double l = in[0], m = in[1], bmaj = in[6], bmin = in[7], bpa = in[8];
        double f[4] = {0.0, 0.0, 0.0, 0.0};
        bool ok = is_fin(l) && is_fin(m) && is_fin(bmaj) && is_fin(bmin) && is_fin(bpa);
        for (int t = 0; t < T; ++t) {
            f[t] = in[2 + t];
            ok = ok && is_fin(f[t]);
        }
        const double r2 = l * l + m * m;
        ok = ok && !(r2 > 1.0) && !(bmaj < bmin) && !(bmin < 0.0);
        double o[DFT_PREP] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (ok) {
            o[0] = l, o[1] = m;
            o[2] = -r2 / (1.0 + sqrt(1.0 - r2));  // n - 1 without the cancellation of the subtraction
            o[3] = f[0], o[4] = f[1], o[5] = f[2], o[6] = f[3];
            if (bmaj != 0.0 || bmin != 0.0) {
                // bmaj^2 up^2 + bmin^2 vp^2 with up = u s + v c, vp = u c - v s, as a quadratic form in (u, v)
                const double k = 9.869604401089358 / (4.0 * 0.6931471805599453);  // pi^2 / (4 ln 2)
                const double s = sin(bpa), cs = cos(bpa), a2 = bmaj * bmaj, b2 = bmin * bmin;
                o[7] = k * (a2 * s * s + b2 * cs * cs);
                o[8] = k * (2.0 * (a2 - b2) * s * cs);
                o[9] = k * (a2 * cs * cs + b2 * s * s);
                // an axis so large that its square overflows (above about 1e154): the form is not finite - skipped
                ok = is_fin(o[7]) && is_fin(o[8]) && is_fin(o[9]);
                if (!ok)
                    for (int j = 0; j < DFT_PREP; ++j) o[j] = 0.0;
            }
        }
        if (!ok) skip += 1.0;
        double *out = prep + c * DFT_PREP;
        for (int j = 0; j < DFT_PREP; ++j) out[j] = o[j];
    }
    skip = block_sum256(skip, lds);
    if (threadIdx.x == 0) skipped[blockIdx.x] = skip;
}

// S(x) by Horner, every product rounded; TT: the terms in use (1 when x is not given)
template <int TT>
__device__ __forceinline__ double flux_at(const double *__restrict__ c, double x)
{
#pragma clang fp contract(off)
    double s = c[3 + TT - 1];
#pragma unroll
    for (int t = TT - 2; t >= 0; --t) {
        const double sx = x * s;
        s = c[3 + t] + sx;
    }
    return s;
}

// One term: acc += amp * exp(-2 pi i p).  The reduction to r is exact (p - rint(p) is representable), |2 r| <= 1.
__device__ __forceinline__ void add_term(double u, double v, double w, const double *__restrict__ c, double amp, double2 &acc)
{
    const double p = fma(w, c[2], fma(v, c[1], u * c[0]));
    const double r = p - rint(p);
    double sn, cs;
    sincospi(2.0 * r, &sn, &cs);
    acc.x = fma(amp, cs, acc.x);
    acc.y = fma(-amp, sn, acc.y);
}

// per: the components of a slice (the same for every slice; the last may be short or empty).  SLICED: the sums go to
// part[blockIdx.y][k]; else vis_out[k] = the sum, or vis_sub[k] - it.  bad[b]: the visibilities of work-group b whose
// coordinates are not finite (written by slice 0).  vis_sub may be vis_out: no __restrict__ on either.
template <int TT, bool SLICED>
__global__ void __launch_bounds__(DFT_BLOCK)
    dft_main_kernel(int64_t n, const double *__restrict__ u, const double *__restrict__ v, const double *__restrict__ w,
                    int64_t stride, const double *__restrict__ x, const double *__restrict__ prep,
                    const int64_t *__restrict__ head, int64_t per, const double2 *vis_sub, double2 *vis_out,
                    double2 *__restrict__ part, double *__restrict__ bad)
{
    __shared__ double comp[DFT_CHUNK * DFT_PREP];
    __shared__ double lds[4];
    const int64_t use = head[0];
    int64_t c0 = (int64_t)blockIdx.y * per, c1 = c0 + per;
    if (c1 > use) c1 = use;
    double uu[2], vv[2], ww[2], xx[2];
    bool live[2], isbad[2];
    double2 acc[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int64_t k = (int64_t)blockIdx.x * DFT_WG_VIS + threadIdx.x + j * DFT_BLOCK;
        live[j] = k < n;
        uu[j] = vv[j] = ww[j] = xx[j] = 0.0;
        if (live[j]) {
            uu[j] = u[k * stride], vv[j] = v[k * stride];
            if (w) ww[j] = w[k * stride];
            if (x) xx[j] = x[k];
        }
        isbad[j] = !(is_fin(uu[j]) && is_fin(vv[j]) && is_fin(ww[j]) && is_fin(xx[j]));
        if (isbad[j]) uu[j] = vv[j] = ww[j] = xx[j] = 0.0;  // (the loop runs on zeros; the result is replaced by 0)
        acc[j] = make_double2(0.0, 0.0);
    }
    for (int64_t base = c0; base < c1; base += DFT_CHUNK) {
        const int cnt = (int)(c1 - base < DFT_CHUNK ? c1 - base : DFT_CHUNK);
        __syncthreads();  // (the last chunk has been read)
        for (int e = threadIdx.x; e < cnt * DFT_PREP; e += DFT_BLOCK) comp[e] = prep[base * DFT_PREP + e];
        __syncthreads();
        for (int i = 0; i < cnt; ++i) {
            const double *c = comp + i * DFT_PREP;
            const double quu = c[7], quv = c[8], qvv = c[9];
            if (quu != 0.0 || quv != 0.0 || qvv != 0.0) {  // wave-uniform: every lane reads the same component
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const double q = fma(quu * uu[j], uu[j], fma(quv * uu[j], vv[j], qvv * vv[j] * vv[j]));
                    add_term(uu[j], vv[j], ww[j], c, flux_at<TT>(c, xx[j]) * exp(-q), acc[j]);
                }
            } else {
#pragma unroll
                for (int j = 0; j < 2; ++j) add_term(uu[j], vv[j], ww[j], c, flux_at<TT>(c, xx[j]), acc[j]);
            }
        }
    }
    double nbad = 0.0;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int64_t k = (int64_t)blockIdx.x * DFT_WG_VIS + threadIdx.x + j * DFT_BLOCK;
        if (!live[j]) continue;
        if (isbad[j]) {
            acc[j] = make_double2(0.0, 0.0);
            nbad += 1.0;
        }
        if (SLICED) {
            part[(int64_t)blockIdx.y * n + k] = acc[j];
        } else if (vis_sub) {
            const double2 s = vis_sub[k];
            vis_out[k] = make_double2(s.x - acc[j].x, s.y - acc[j].y);
        } else {
            vis_out[k] = acc[j];
        }
    }
    if (blockIdx.y == 0) {
        nbad = block_sum256(nbad, lds);
        if (threadIdx.x == 0) bad[blockIdx.x] = nbad;
    }
}

__global__ void __launch_bounds__(256)
    dft_epilogue_kernel(int64_t n, int S, const double2 *__restrict__ part, const double2 *vis_sub, double2 *vis_out)
{
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x) {
        double2 a = part[k];
        for (int s = 1; s < S; ++s) {
            const double2 b = part[(int64_t)s * n + k];
            a.x += b.x, a.y += b.y;
        }
        if (vis_sub) {
            const double2 s = vis_sub[k];
            a = make_double2(s.x - a.x, s.y - a.y);
        }
        vis_out[k] = a;
    }
}

// C == 0 or nothing to sum: vis_out = 0, or vis_sub
__global__ void __launch_bounds__(256) dft_empty_kernel(int64_t n, const double2 *vis_sub, double2 *vis_out)
{
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x)
        vis_out[k] = vis_sub ? vis_sub[k] : make_double2(0.0, 0.0);
}

// the non-finite visibilities of a call that ran no main kernel (C == 0), one row per work-group
__global__ void __launch_bounds__(DFT_BLOCK)
    dft_badvis_kernel(int64_t n, const double *__restrict__ u, const double *__restrict__ v, const double *__restrict__ w,
                      int64_t stride, const double *__restrict__ x, double *__restrict__ bad)
{
    __shared__ double lds[4];
    double nbad = 0.0;
    for (int64_t k = (int64_t)blockIdx.x * DFT_BLOCK + threadIdx.x; k < n; k += (int64_t)gridDim.x * DFT_BLOCK) {
        const bool ok = is_fin(u[k * stride]) && is_fin(v[k * stride]) && (!w || is_fin(w[k * stride])) && (!x || is_fin(x[k]));
        nbad += ok ? 0.0 : 1.0;
    }
    nbad = block_sum256(nbad, lds);
    if (threadIdx.x == 0) bad[blockIdx.x] = nbad;
}

__global__ void __launch_bounds__(DFT_BLOCK)
    dft_stats_kernel(int64_t nskip, const double *__restrict__ skipped, int64_t nbad, const double *__restrict__ bad,
                     const int64_t *__restrict__ head, int S, double *__restrict__ stats)
{
    __shared__ double lds[4];
    double a = 0.0, b = 0.0;
    for (int64_t i = threadIdx.x; i < nskip; i += DFT_BLOCK) a += skipped[i];
    for (int64_t i = threadIdx.x; i < nbad; i += DFT_BLOCK) b += bad[i];
    a = block_sum256(a, lds);
    b = block_sum256(b, lds);
    if (threadIdx.x != 0) return;
    stats[0] = (double)head[0] - a;
    stats[1] = a;
    stats[2] = b;
    stats[3] = (double)S;
}

// ---- components from a model image ----------------------------------------------------------------------------------------
__device__ __forceinline__ bool cell_set(const double *__restrict__ model, int64_t cells, int T, int64_t e)
{
    bool nz = false;
    for (int t = 0; t < T; ++t) nz = nz || model[(int64_t)t * cells + e] != 0.0;  // (NaN is not zero)
    return nz;
}

// (block_rank and CFI_SEG are in imaging.h: sources.hip compacts the island roots the same way)
__global__ void __launch_bounds__(256)
    cfi_count_kernel(int64_t cells, int T, const double *__restrict__ model, int64_t nseg, unsigned int *__restrict__ segcount)
{
    __shared__ unsigned int lds[4];
    for (int64_t seg = blockIdx.x; seg < nseg; seg += gridDim.x) {
        unsigned int mine = 0;
        for (int j = 0; j < 4; ++j) {
            const int64_t e = seg * CFI_SEG + 4 * threadIdx.x + j;
            if (e < cells && cell_set(model, cells, T, e)) ++mine;
        }
        unsigned int total;
        block_rank(mine, lds, &total);
        if (threadIdx.x == 0) segcount[seg] = total;
    }
}

// one work-group of 1024 threads: thread i takes the segments [i * each, (i + 1) * each); offs = the exclusive scan
__global__ void __launch_bounds__(1024)
    cfi_scan_kernel(int64_t nseg, const unsigned int *__restrict__ segcount, int64_t *__restrict__ offs,
                    int64_t *__restrict__ count)
{
    __shared__ long long sums[1024];
    const int64_t each = (nseg + 1023) / 1024, s0 = threadIdx.x * each, s1 = s0 + each < nseg ? s0 + each : nseg;
    long long mine = 0;
    for (int64_t s = s0; s < s1; ++s) mine += segcount[s];
    sums[threadIdx.x] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long run = 0;
        for (int i = 0; i < 1024; ++i) {
            const long long t = sums[i];
            sums[i] = run;
            run += t;
        }
        *count = run;
    }
    __syncthreads();
    long long run = sums[threadIdx.x];
    for (int64_t s = s0; s < s1; ++s) {
        offs[s] = run;
        run += segcount[s];
    }
}

__global__ void __launch_bounds__(256)
    cfi_scatter_kernel(int64_t N, int T, double theta, const double *__restrict__ model, int64_t nseg,
                       const int64_t *__restrict__ offs, int64_t max_c, double *__restrict__ comps)
{
#pragma clang fp contract(off)
    __shared__ unsigned int lds[4];
    const int64_t cells = N * N, half = N / 2;
    for (int64_t seg = blockIdx.x; seg < nseg; seg += gridDim.x) {
        unsigned int mine = 0;
        bool set[4];
        for (int j = 0; j < 4; ++j) {
            const int64_t e = seg * CFI_SEG + 4 * threadIdx.x + j;
            set[j] = e < cells && cell_set(model, cells, T, e);
            mine += set[j];
        }
        unsigned int total;
        int64_t row = offs[seg] + block_rank(mine, lds, &total);
        for (int j = 0; j < 4; ++j) {
            if (!set[j]) continue;
            if (row < max_c) {
                const int64_t e = seg * CFI_SEG + 4 * threadIdx.x + j, y = e / N, x = e - y * N;
                double *o = comps + row * GRIDHIP_COMP_DOUBLES;
                o[0] = theta * (double)(x - half) / (double)N;
                o[1] = theta * (double)(y - half) / (double)N;
                for (int t = 0; t < 4; ++t) o[2 + t] = t < T ? model[(int64_t)t * cells + e] : 0.0;
                o[6] = 0.0, o[7] = 0.0, o[8] = 0.0, o[9] = 0.0;
            }
            ++row;
        }
    }
}

template <int TT>
void launch_main(gridhip_ctx *ctx, dim3 grid, bool sliced, int64_t n, const double *u, const double *v, const double *w,
                 int64_t stride, const double *x, const double *prep, const int64_t *head, int64_t per,
                 const double2 *vis_sub, double2 *vis_out, double2 *part, double *bad)
{
    if (sliced)
        hipLaunchKernelGGL((dft_main_kernel<TT, true>), grid, dim3(DFT_BLOCK), 0, ctx->stream, n, u, v, w, stride, x, prep,
                           head, per, vis_sub, vis_out, part, bad);
    else
        hipLaunchKernelGGL((dft_main_kernel<TT, false>), grid, dim3(DFT_BLOCK), 0, ctx->stream, n, u, v, w, stride, x, prep,
                           head, per, vis_sub, vis_out, part, bad);
}

}  // namespace

int dft_slices(gridhip_ctx *ctx, int64_t n, int64_t C)
{
    const int64_t forced = ctx->img->dft_slices;
    if (forced >= 1) return (int)(forced > DFT_MAX_SLICES ? DFT_MAX_SLICES : forced);
    const int64_t groups = (n + DFT_WG_VIS - 1) / DFT_WG_VIS, chunks = (C + DFT_CHUNK - 1) / DFT_CHUNK;
    if (groups < 1 || groups >= DFT_FILL / 2 || chunks < 2) return 1;
    int64_t S = DFT_FILL / groups;  // (a slice takes at least one chunk's worth of components)
    if (S > chunks) S = chunks;
    if (S > DFT_MAX_SLICES) S = DFT_MAX_SLICES;
    return (int)(S < 1 ? 1 : S);
}

int dft_predict_check(gridhip_ctx *ctx, int64_t C, const double *comps, const int64_t *count, int T, int64_t n,
                      const double *u, const double *v, const double *w, int64_t stride, const double *x,
                      const double *vis_sub, const double *vis_out, const double *stats)
{
    if (n < 0 || C < 0 || T < 1 || T > 4 || (C > 0 && !comps) || (n > 0 && (!u || !v || !vis_out)) || stride < 1)
        return fail(ctx, GRIDHIP_EINVAL, "dft_predict: n >= 0, C >= 0, T in 1..4, comps, u, v, vis_out, uv_stride >= 1");
    if (n > (int64_t)0x7fffff00) return fail(ctx, GRIDHIP_EUNSUPPORTED, "dft_predict: n must be < 2^31 per call");
    const size_t ob = (size_t)n * 16, sb = span_bytes(n, stride), cb = (size_t)C * GRIDHIP_COMP_DOUBLES * 8;
    if (overlaps_any({vis_out, ob}, {{comps, cb}, {count, 8}, {u, sb}, {v, sb}, {w, sb}, {x, (size_t)n * 8}}) ||
        (vis_out != vis_sub && overlap(vis_out, ob, vis_sub, ob)))
        return fail(ctx, GRIDHIP_EINVAL, "dft_predict: vis_out may be vis_sub itself, and overlap nothing else");
    if (overlaps_any({stats, 32}, {{vis_out, ob}, {vis_sub, ob}, {comps, cb}, {count, 8}, {u, sb}, {v, sb}, {w, sb},
                                   {x, (size_t)n * 8}}))
        return fail(ctx, GRIDHIP_EINVAL, "dft_predict: stats overlaps another argument");
    return GRIDHIP_OK;
}

int dft_predict_run(gridhip_ctx *ctx, int64_t C, const double *comps, const int64_t *count_dev, int T, int64_t n,
                    const double *u, const double *v, const double *w, int64_t stride, const double *x,
                    const double *vis_sub, double *vis_out, double *stats)
{
    if (n == 0 && !stats) return GRIDHIP_OK;
    const int S = n > 0 && C > 0 ? dft_slices(ctx, n, C) : 1;
    const int64_t groups = (n + DFT_WG_VIS - 1) / DFT_WG_VIS;
    const dim3 pgrid = grid_for(ctx, C), bgrid = grid_for(ctx, n, DFT_BLOCK);
    const int64_t nbad = n == 0 ? 0 : (C > 0 ? groups : (int64_t)bgrid.x);
    DevBuf prep, small, part;
    GH_CHECK(prep.alloc(ctx, (size_t)C * DFT_PREP * 8));
    GH_CHECK(small.alloc(ctx, (8 + (size_t)pgrid.x + (size_t)(groups > (int64_t)bgrid.x ? groups : (int64_t)bgrid.x)) * 8));
    if (S > 1) GH_CHECK(part.alloc(ctx, (size_t)S * n * 16));
    int64_t *head = small.as<int64_t>();
    double *skipped = small.as<double>() + 8, *bad = skipped + pgrid.x;
    hipLaunchKernelGGL(dft_prepare_kernel, pgrid, dim3(DFT_BLOCK), 0, ctx->stream, C, comps, count_dev, T, prep.as<double>(),
                       head, skipped);
    if (n > 0 && C > 0) {
        const int64_t per = (C + S - 1) / S;
        const dim3 grid((unsigned)groups, (unsigned)S);
        const int TT = x ? T : 1;
        auto go = TT == 1 ? launch_main<1> : TT == 2 ? launch_main<2> : TT == 3 ? launch_main<3> : launch_main<4>;
        go(ctx, grid, S > 1, n, u, v, w, stride, x, prep.as<double>(), head, per, (const double2 *)vis_sub,
           (double2 *)vis_out, part.as<double2>(), bad);
        if (S > 1)
            hipLaunchKernelGGL(dft_epilogue_kernel, grid_for(ctx, n), dim3(256), 0, ctx->stream, n, S,
                               (const double2 *)part.as<double2>(), (const double2 *)vis_sub, (double2 *)vis_out);
    } else if (n > 0) {
        if (vis_out != vis_sub)
            hipLaunchKernelGGL(dft_empty_kernel, grid_for(ctx, n), dim3(256), 0, ctx->stream, n, (const double2 *)vis_sub,
                               (double2 *)vis_out);
        if (stats)
            hipLaunchKernelGGL(dft_badvis_kernel, bgrid, dim3(DFT_BLOCK), 0, ctx->stream, n, u, v, w, stride, x, bad);
    }
    if (stats)
        hipLaunchKernelGGL(dft_stats_kernel, dim3(1), dim3(DFT_BLOCK), 0, ctx->stream, (int64_t)pgrid.x,
                           (const double *)skipped, nbad, (const double *)bad, (const int64_t *)head, S, stats);
    GH_CHECK_HIP(ctx, hipGetLastError());
    return GRIDHIP_OK;
}

int components_check(gridhip_ctx *ctx, double theta, int64_t lam, int T, const double *model, int64_t max_c,
                     const double *comps, const int64_t *count, int64_t *N)
{
    *N = gridhip_image_size(theta, lam);
    if (*N < 1 || T < 1 || T > 4 || !model || max_c < 0 || !count || (max_c > 0 && !comps))
        return fail(ctx, GRIDHIP_EINVAL, "components_from_image: an image size >= 1, T in 1..4, model, max_c >= 0, comps, count");
    if (*N > ((int64_t)1 << 20)) return fail(ctx, GRIDHIP_EUNSUPPORTED, "components_from_image: N above 2^20");
    const size_t mb = (size_t)T * *N * *N * 8, cb = (size_t)max_c * GRIDHIP_COMP_DOUBLES * 8;
    if (overlap(comps, cb, model, mb) || overlap(count, 8, model, mb) || overlap(count, 8, comps, cb))
        return fail(ctx, GRIDHIP_EINVAL, "components_from_image: comps, count and model must not overlap");
    return GRIDHIP_OK;
}

int segment_scan(gridhip_ctx *ctx, int64_t nseg, const unsigned int *segcount, int64_t *offs, int64_t *count)
{
    hipLaunchKernelGGL(cfi_scan_kernel, dim3(1), dim3(1024), 0, ctx->stream, nseg, segcount, offs, count);
    GH_CHECK_HIP(ctx, hipGetLastError());
    return GRIDHIP_OK;
}

int components_run(gridhip_ctx *ctx, int64_t N, double theta, int T, const double *model, int64_t max_c, double *comps,
                   int64_t *count_dev)
{
    const int64_t cells = N * N, nseg = (cells + CFI_SEG - 1) / CFI_SEG;
    DevBuf segcount, offs;
    GH_CHECK(segcount.alloc(ctx, (size_t)nseg * 4));
    GH_CHECK(offs.alloc(ctx, (size_t)nseg * 8));
    const dim3 grid = grid_for(ctx, nseg, 1);
    hipLaunchKernelGGL(cfi_count_kernel, grid, dim3(256), 0, ctx->stream, cells, T, model, nseg, segcount.as<unsigned int>());
    GH_CHECK(segment_scan(ctx, nseg, segcount.as<unsigned int>(), offs.as<int64_t>(), count_dev));
    if (max_c > 0)
        hipLaunchKernelGGL(cfi_scatter_kernel, grid, dim3(256), 0, ctx->stream, N, T, theta, model, nseg,
                           (const int64_t *)offs.as<int64_t>(), max_c, comps);
    GH_CHECK_HIP(ctx, hipGetLastError());
    return GRIDHIP_OK;
}

}  // namespace gridhip

using namespace gridhip;

namespace {

int dft_predict_any(gridhip_ctx *ctx, bool dev, int64_t C, const double *comps, const int64_t *count, int T, int64_t n,
                    const double *u, const double *v, const double *w, int64_t uv_stride, const double *x,
                    const double *vis_sub, double *vis_out, double *stats)
{
    if (!ctx) return GRIDHIP_EINVAL;
    GH_CHECK(dft_predict_check(ctx, C, comps, count, T, n, u, v, w, uv_stride, x, vis_sub, vis_out, stats));
    GH_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    const size_t sb = span_bytes(n, uv_stride), ob = (size_t)n * 16;
    Staged st(ctx, dev);
    comps = st.in(comps, (size_t)C * GRIDHIP_COMP_DOUBLES * 8), count = st.in(count, 8), u = st.in(u, sb), v = st.in(v, sb);
    w = st.in(w, sb), x = st.in(x, (size_t)n * 8), vis_sub = st.in(vis_sub, ob), vis_out = st.out(vis_out, ob);
    stats = st.out(stats, 32);
    GH_CHECK(st.status());
    GH_CHECK(dft_predict_run(ctx, C, comps, count, T, n, u, v, w, uv_stride, x, vis_sub, vis_out, stats));
    return st.finish();
}

int components_any(gridhip_ctx *ctx, bool dev, double theta, int64_t lam, int T, const double *model, int64_t max_c,
                   double *comps, int64_t *count)
{
    if (!ctx) return GRIDHIP_EINVAL;
    int64_t N = 0;
    GH_CHECK(components_check(ctx, theta, lam, T, model, max_c, comps, count, &N));
    GH_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    Staged st(ctx, dev);
    model = st.in(model, (size_t)T * N * N * 8);
    double *dc = st.raw(comps, (size_t)max_c * GRIDHIP_COMP_DOUBLES * 8);
    int64_t *dn = st.raw(count, 8);
    GH_CHECK(st.status());
    GH_CHECK(components_run(ctx, N, theta, T, model, max_c, dc, dn));
    if (dev) return GRIDHIP_OK;
    // only the rows written come back: the caller's rows after them stay as they were
    int64_t found = 0;
    GH_CHECK(d2h(ctx, &found, dn, 8));
    GH_CHECK(sync(ctx));
    GH_CHECK(d2h(ctx, comps, dc, (size_t)(found < max_c ? found : max_c) * GRIDHIP_COMP_DOUBLES * 8));
    GH_CHECK(st.finish());
    *count = found;
    return GRIDHIP_OK;
}

}  // namespace

extern "C" {

int gridhip_dft_predict_dev(gridhip_ctx *ctx, int64_t C, const double *comps, const int64_t *count_dev, int T, int64_t n,
                            const double *u, const double *v, const double *w, int64_t uv_stride, const double *x,
                            const double *vis_sub, double *vis_out, double *stats)
{
    return dft_predict_any(ctx, true, C, comps, count_dev, T, n, u, v, w, uv_stride, x, vis_sub, vis_out, stats);
}

int gridhip_dft_predict(gridhip_ctx *ctx, int64_t C, const double *comps, const int64_t *count, int T, int64_t n,
                        const double *u, const double *v, const double *w, int64_t uv_stride, const double *x,
                        const double *vis_sub, double *vis_out, double *stats)
{
    return dft_predict_any(ctx, false, C, comps, count, T, n, u, v, w, uv_stride, x, vis_sub, vis_out, stats);
}

int gridhip_components_from_image_dev(gridhip_ctx *ctx, double theta, int64_t lam, int T, const double *model,
                                      int64_t max_c, double *comps, int64_t *count)
{
    return components_any(ctx, true, theta, lam, T, model, max_c, comps, count);
}

int gridhip_components_from_image(gridhip_ctx *ctx, double theta, int64_t lam, int T, const double *model, int64_t max_c,
                                  double *comps, int64_t *count)
{
    return components_any(ctx, false, theta, lam, T, model, max_c, comps, count);
}

}  // extern "C"
