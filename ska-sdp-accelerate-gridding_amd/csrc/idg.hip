// Image-domain layers of a w-stack (include/gridhip.h, "w-stacking", IMAGE-DOMAIN LAYERS): the partition of a stream by
// (layer, tile) and the two kernels that stand in a layer's gridder and degridder.  No kernel table, no LDS atomics: the
// gridder's hot loop is one fp64 sincospi and a complex multiply-add per (visibility, subgrid pixel), the pixels in
// registers and the visibilities broadcast from LDS.
#include "idg.h"

namespace gridhip {

namespace {

// The cell coordinate x = N p + N div 2 of p = u / lam, its tile t = floor(x) div T (floor(x / T), without the rounding of
// that quotient) and a = x - cx, cx = t T - K / 2 + Sg / 2.  False: outside 0 <= x < N, or NaN.  Both sweeps of the
// partition go through here, so they agree on every visibility.
__device__ __forceinline__ bool idg_cell(double p, int64_t N, int Sg, int K, int *t, double *a)
{
#pragma clang fp contract(off)
    const double x = (double)N * p + (double)(N / 2);
    if (!(x >= 0.0 && x < (double)N)) return false;
    const int T = Sg - K;
    *t = (int)((int64_t)floor(x) / T);
    *a = x - (double)(*t * T - K / 2 + Sg / 2);
    return true;
}

struct IdgPart {
    int64_t n, stride, N, M;
    const double *u, *v, *w;
    double lam, wstep, pmin;
    int L, Sg, K, nt;
};

// the key l nt^2 + ty nt + tx of visibility k, or -1 where it is dropped
__device__ __forceinline__ int64_t idg_key(const IdgPart &p, int64_t k, double *a, double *b, double *dw)
{
    const double w = p.w[k * p.stride];
    int64_t r;
    const int l = layer_of(w, p.wstep, p.pmin, p.M, &r);
    if (l < 0 || l >= p.L) return -1;
    int tx, ty;
    if (!idg_cell(p.u[k * p.stride] / p.lam, p.N, p.Sg, p.K, &tx, a)) return -1;
    if (!idg_cell(p.v[k * p.stride] / p.lam, p.N, p.Sg, p.K, &ty, b)) return -1;
    const int64_t pc = (int64_t)p.pmin + (int64_t)l * p.M + p.M / 2;
    *dw = w - (double)pc * p.wstep;
    return ((int64_t)l * p.nt + ty) * p.nt + tx;
}

__global__ void __launch_bounds__(256) idg_count_kernel(IdgPart p, int32_t *__restrict__ count)
{
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < p.n; k += (int64_t)gridDim.x * blockDim.x) {
        double a, b, dw;
        const int64_t key = idg_key(p, k, &a, &b, &dw);
        if (key >= 0) atomicAdd(&count[key], 1);
    }
}

// offs[0 .. nkeys] = the exclusive scan of count and its total, cursor = offs, ioffs[0 .. nkeys] = the scan of the work
// items ceil(count / IDG_SPLIT) of every key: one work-group, a run of keys per thread
__global__ void __launch_bounds__(256) idg_scan_kernel(int64_t nkeys, const int32_t *__restrict__ count,
                                                       int32_t *__restrict__ offs, int32_t *__restrict__ cursor,
                                                       int32_t *__restrict__ ioffs)
{
    __shared__ unsigned int lds[4];
    const int64_t per = (nkeys + 255) / 256, lo = threadIdx.x * per;
    unsigned int mine = 0, items = 0;
    for (int64_t i = lo; i < lo + per && i < nkeys; ++i) {
        const unsigned int c = (unsigned int)count[i];
        mine += c;
        items += (c + IDG_SPLIT - 1) / IDG_SPLIT;
    }
    unsigned int total, itotal;
    unsigned int run = block_rank(mine, lds, &total);
    unsigned int irun = block_rank(items, lds, &itotal);
    for (int64_t i = lo; i < lo + per && i < nkeys; ++i) {
        const unsigned int c = (unsigned int)count[i];
        offs[i] = (int32_t)run;
        cursor[i] = (int32_t)run;
        ioffs[i] = (int32_t)irun;
        run += c;
        irun += (c + IDG_SPLIT - 1) / IDG_SPLIT;
    }
    if (threadIdx.x == 0) offs[nkeys] = (int32_t)total, ioffs[nkeys] = (int32_t)itotal;
}

// bounds[2 l], bounds[2 l + 1] = offs, ioffs at the first key of layer l, l = 0 .. L: what the host reads back
__global__ void __launch_bounds__(256) idg_bounds_kernel(int L, int64_t nt2, const int32_t *__restrict__ offs,
                                                         const int32_t *__restrict__ ioffs, int32_t *__restrict__ bounds)
{
    for (int l = blockIdx.x * blockDim.x + threadIdx.x; l <= L; l += gridDim.x * blockDim.x)
        bounds[2 * l] = offs[l * nt2], bounds[2 * l + 1] = ioffs[l * nt2];
}

__global__ void __launch_bounds__(256) idg_scatter_kernel(IdgPart p, int32_t *__restrict__ cursor, int64_t cap,
                                                          double *__restrict__ oa, double *__restrict__ ob,
                                                          double *__restrict__ odw, int32_t *__restrict__ src)
{
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < p.n; k += (int64_t)gridDim.x * blockDim.x) {
        double a, b, dw;
        const int64_t key = idg_key(p, k, &a, &b, &dw);
        if (key < 0) continue;
        const int64_t pos = atomicAdd(&cursor[key], 1);
        if (pos < 0 || pos >= cap) continue;  // (cannot happen: the counts are of this very rule)
        oa[pos] = a;
        ob[pos] = b;
        odw[pos] = dw;
        src[pos] = (int32_t)k;
    }
}

// the work items of every occupied key, at ioffs[key]
__global__ void __launch_bounds__(256) idg_items_kernel(int64_t nkeys, int nt, int Sg, int K, const int32_t *__restrict__ count,
                                                        const int32_t *__restrict__ offs, const int32_t *__restrict__ ioffs,
                                                        int64_t nitems, IdgItem *__restrict__ items)
{
    const int T = Sg - K;
    for (int64_t key = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; key < nkeys; key += (int64_t)gridDim.x * blockDim.x) {
        const int32_t c = count[key];
        if (c <= 0) continue;
        const int64_t tile = key % ((int64_t)nt * nt);
        const int ty = (int)(tile / nt), tx = (int)(tile - (int64_t)ty * nt);
        int64_t at = ioffs[key];
        for (int32_t done = 0; done < c && at < nitems; done += IDG_SPLIT, ++at) {
            IdgItem it;
            it.ox = tx * T - K / 2, it.oy = ty * T - K / 2;
            it.off = offs[key] + done;
            it.cnt = c - done < IDG_SPLIT ? c - done : IDG_SPLIT;
            items[at] = it;
        }
    }
}

// ---- the subgrid's geometry, per thread ------------------------------------------------------------------------------------
// A work-group of 256 threads holds the SG^2 pixels in registers: pixel t + 256 e of thread t, e < PP (1, 3, 4: at SG = 24
// the third is a pixel for the first 64 threads only).
template <int SG>
struct IdgPix {
    static constexpr int PIX = SG * SG, PP = (PIX + 255) / 256, H = SG / 2;
};

// f_i = (i - SG / 2) / SG; ph = 1 - sqrt(1 - l_i^2 - l_j^2), l = f theta; false where l_i^2 + l_j^2 >= 1 (the pixel counts 0)
template <int SG>
__device__ __forceinline__ bool idg_pixel(int pix, double theta, double *fi, double *fj, double *ph)
{
    const int j = pix / SG, i = pix - j * SG;
    *fi = (double)(i - SG / 2) / (double)SG;
    *fj = (double)(j - SG / 2) / (double)SG;
    const double li = *fi * theta, lj = *fj * theta;
    const double r2 = li * li + lj * lj;
    *ph = r2 < 1.0 ? 1.0 - sqrt(1.0 - r2) : 0.0;
    return r2 < 1.0;
}

// root[m] = e(-m / SG), m < SG
template <int SG>
__device__ __forceinline__ void idg_roots(double2 *root)
{
    if (threadIdx.x < SG) {
        double s, c;
        sincospi(-2.0 * (double)threadIdx.x / (double)SG, &s, &c);
        root[threadIdx.x] = make_double2(c, s);
    }
}

// sum_i in[i * stride] e(-+ (p - H) (i - H) / SG): one output of an SG-point centred DFT from the table of roots; CONJ: e(+)
template <int SG, bool CONJ>
__device__ __forceinline__ double2 idg_dft1(const double2 *in, int stride, int p, const double2 *root)
{
    constexpr int H = SG / 2;
    int step = (p - H) % SG;
    step += step < 0 ? SG : 0;
    int m = (step * (SG - H)) % SG;  // (p - H) (0 - H) mod SG
    double2 acc = make_double2(0.0, 0.0);
    for (int i = 0; i < SG; ++i) {
        const double2 z = in[i * stride];
        double2 r = root[m];
        if (CONJ) r.y = -r.y;
        acc.x += z.x * r.x - z.y * r.y;
        acc.y += z.x * r.y + z.y * r.x;
        m += step;
        m -= m >= SG ? SG : 0;
    }
    return acc;
}

// The gridder: one work-group per work item.  Every thread sums its pixels over the item's visibilities, which come
// through LDS in chunks of IDG_CHUNK records (a, b, dw, re, im) that all lanes read at the same address (a broadcast).
// Then the taper, the separable SG-point DFT on both axes in LDS, and the clipped flush with fp64 atomic adds: subgrids
// of neighbouring tiles overlap in their margins, and a split tile's pieces land on the same cells.
template <int SG>
__global__ void __launch_bounds__(256) idg_grid_kernel(const IdgItem *__restrict__ items, const double *__restrict__ a,
                                                       const double *__restrict__ b, const double *__restrict__ dw,
                                                       const double2 *__restrict__ vis, double theta, int K, int64_t N,
                                                       double *__restrict__ grid)
{
    using G = IdgPix<SG>;
    constexpr int PIX = G::PIX, PP = G::PP;
    constexpr int NB = PIX > (IDG_CHUNK * 5) / 2 ? PIX : (IDG_CHUNK * 5) / 2;
    __shared__ double2 sA[PIX];
    __shared__ double2 sB[NB];  // the chunk's five rows of IDG_CHUNK doubles, later the DFT's second buffer
    __shared__ double2 root[SG];
    const IdgItem it = items[blockIdx.x];
    const int t = threadIdx.x;
    double fi[PP], fj[PP], ph[PP];
    bool ok[PP];
    double2 acc[PP];
#pragma unroll
    for (int e = 0; e < PP; ++e) {
        const int pix = t + 256 * e;
        ok[e] = idg_pixel<SG>(pix < PIX ? pix : 0, theta, &fi[e], &fj[e], &ph[e]) && pix < PIX;
        acc[e] = make_double2(0.0, 0.0);
    }
    idg_roots<SG>(root);
    double *ca = (double *)sB, *cb = ca + IDG_CHUNK, *cw = cb + IDG_CHUNK, *cr = cw + IDG_CHUNK, *ci = cr + IDG_CHUNK;
    for (int c0 = 0; c0 < it.cnt; c0 += IDG_CHUNK) {
        const int m = it.cnt - c0 < IDG_CHUNK ? it.cnt - c0 : IDG_CHUNK;
        __syncthreads();
        if (t < m) {
            const int64_t j = (int64_t)it.off + c0 + t;
            const double2 z = vis[j];
            ca[t] = a[j], cb[t] = b[j], cw[t] = dw[j], cr[t] = z.x, ci[t] = z.y;
        }
        __syncthreads();
        for (int r = 0; r < m; ++r) {
            const double A = ca[r], B = cb[r], W = cw[r], re = cr[r], im = ci[r];
#pragma unroll
            for (int e = 0; e < PP; ++e) {
                const double p = A * fi[e] + B * fj[e] - W * ph[e];
                double s, c;
                sincospi(2.0 * (p - rint(p)), &s, &c);
                acc[e].x += re * c - im * s;
                acc[e].y += re * s + im * c;
            }
        }
    }
    // the taper; a pixel beyond the horizon counts 0
#pragma unroll
    for (int e = 0; e < PP; ++e) {
        const int pix = t + 256 * e;
        const double tp = ok[e] ? idg_taper(fi[e], K) * idg_taper(fj[e], K) : 0.0;
        if (pix < PIX) sA[pix] = ok[e] ? make_double2(acc[e].x * tp, acc[e].y * tp) : make_double2(0.0, 0.0);
    }
    __syncthreads();  // (also: the last chunk has been read by every thread, sB is free)
    // along i: X[j][p] = sum_i Pt[j][i] e(-(p - H) f_i)
#pragma unroll
    for (int e = 0; e < PP; ++e) {
        const int pix = t + 256 * e;
        if (pix < PIX) {
            const int j = pix / SG, p = pix - j * SG;
            sB[pix] = idg_dft1<SG, false>(sA + j * SG, 1, p, root);
        }
    }
    __syncthreads();
    // along j: Gs[q][p] = SG^-2 sum_j X[j][p] e(-(q - H) f_j); the flush, clipped at the grid's borders
#pragma unroll
    for (int e = 0; e < PP; ++e) {
        const int pix = t + 256 * e;
        if (pix < PIX) {
            const int q = pix / SG, p = pix - q * SG;
            const double2 g = idg_dft1<SG, false>(sB + p, SG, q, root);
            const int64_t gy = (int64_t)it.oy + q, gx = (int64_t)it.ox + p;
            if (gy >= 0 && gy < N && gx >= 0 && gx < N) {
                const double sc = 1.0 / (double)(SG * SG);
                unsafeAtomicAdd(grid + 2 * (gy * N + gx), g.x * sc);
                unsafeAtomicAdd(grid + 2 * (gy * N + gx) + 1, g.y * sc);
            }
        }
    }
}

// The degridder: one work-group per work item.  The patch of f under the subgrid is read clipped (0 outside the grid),
// goes through the adjoint DFT on both axes and the taper into an LDS subgrid, and every thread then sums a visibility of
// its own over the pixels, j outer and i inner, and writes it at its own slot: no atomics, the same bits every run.
// NT threads per work-group: a work item of few visibilities keeps few lanes busy in the last loop, so the launcher takes
// 64 or 128 threads where a layer's items are small (every pixel and every visibility is still one thread's).
template <int SG, int NT>
__global__ void __launch_bounds__(NT) idg_degrid_kernel(const IdgItem *__restrict__ items, const double *__restrict__ a,
                                                         const double *__restrict__ b, const double *__restrict__ dw,
                                                         double theta, int K, int64_t N, const double2 *__restrict__ f,
                                                         double2 *__restrict__ out)
{
    using G = IdgPix<SG>;
    constexpr int PIX = G::PIX, PP = (PIX + NT - 1) / NT, H = G::H;
    __shared__ double2 sA[PIX];
    __shared__ double2 sB[PIX];
    __shared__ double2 root[SG];
    const IdgItem it = items[blockIdx.x];
    const int t = threadIdx.x;
    idg_roots<SG>(root);
#pragma unroll
    for (int e = 0; e < PP; ++e) {
        const int pix = t + NT * e;
        if (pix < PIX) {
            const int q = pix / SG, p = pix - q * SG;
            const int64_t gy = (int64_t)it.oy + q, gx = (int64_t)it.ox + p;
            sA[pix] = gy >= 0 && gy < N && gx >= 0 && gx < N ? f[gy * N + gx] : make_double2(0.0, 0.0);
        }
    }
    __syncthreads();
    // along p: Y[q][i] = sum_p patch[q][p] e(+(p - H) f_i)
#pragma unroll
    for (int e = 0; e < PP; ++e) {
        const int pix = t + NT * e;
        if (pix < PIX) {
            const int q = pix / SG, i = pix - q * SG;
            sB[pix] = idg_dft1<SG, true>(sA + q * SG, 1, i, root);
        }
    }
    __syncthreads();
    // along q, the taper and the scale into registers; then sA = the subgrid image, sB = ph[j][i]
    double2 pm[PP];
    double phv[PP];
#pragma unroll
    for (int e = 0; e < PP; ++e) {
        const int pix = t + NT * e;
        pm[e] = make_double2(0.0, 0.0);
        phv[e] = 0.0;
        if (pix < PIX) {
            const int j = pix / SG, i = pix - j * SG;
            double fi, fj;
            const bool ok = idg_pixel<SG>(pix, theta, &fi, &fj, &phv[e]);
            const double2 z = idg_dft1<SG, true>(sB + i, SG, j, root);
            const double tp = ok ? idg_taper(fi, K) * idg_taper(fj, K) / (double)(SG * SG) : 0.0;
            if (ok) pm[e] = make_double2(z.x * tp, z.y * tp);
        }
    }
    __syncthreads();
    double *sPh = (double *)sB;
#pragma unroll
    for (int e = 0; e < PP; ++e) {
        const int pix = t + NT * e;
        if (pix < PIX) sA[pix] = pm[e], sPh[pix] = phv[e];
    }
    __syncthreads();
    for (int r = t; r < it.cnt; r += NT) {
        const int64_t k = (int64_t)it.off + r;
        const double A = a[k], B = b[k], W = dw[k];
        double2 acc = make_double2(0.0, 0.0);
#pragma unroll 1
        for (int j = 0; j < SG; ++j) {
            const double bf = B * ((double)(j - H) / (double)SG);
#pragma unroll 2
            for (int i = 0; i < SG; ++i) {
                const double p = A * ((double)(i - H) / (double)SG) + bf - W * sPh[j * SG + i];
                double s, c;
                sincospi(-2.0 * (p - rint(p)), &s, &c);
                const double2 z = sA[j * SG + i];
                acc.x += z.x * c - z.y * s;
                acc.y += z.x * s + z.y * c;
            }
        }
        out[k] = acc;
    }
}

}  // namespace

int idg_partition(gridhip_ctx *ctx, const WStackArgs &args, int64_t N, double pmin, int L, int64_t cap, double *a, double *b,
                  double *dw, int32_t *src, std::vector<IdgSlice> *slices, IdgItem **items)
{
    *items = nullptr;
    slices->clear();
    const int Sg = (int)args.S, K = (int)args.npixFF, T = Sg - K;
    const int64_t nt = (N + T - 1) / T, nt2 = nt * nt, nkeys = (int64_t)L * nt2;
    if (nkeys > IDG_MAX_KEYS)
        return fail(ctx, GRIDHIP_EUNSUPPORTED, "image-domain layers: %lld layers x %lld tiles (at most 2^26): raise planes or wstep",
                    (long long)L, (long long)nt2);
    IdgPart p{args.n, args.stride, N, args.M, args.u, args.v, args.w, (double)args.lam, (double)args.wstep, pmin, L, Sg, K, (int)nt};
    DevBuf tab;  // count[nkeys], offs[nkeys + 1], ioffs[nkeys + 1], cursor[nkeys], bounds[2 (L + 1)]
    GH_CHECK(tab.alloc(ctx, (size_t)(4 * nkeys + 2 + 2 * (L + 1)) * 4));
    int32_t *count = tab.as<int32_t>(), *offs = count + nkeys, *ioffs = offs + nkeys + 1, *cursor = ioffs + nkeys + 1,
            *bounds = cursor + nkeys;
    unsigned g = grid_for(ctx, args.n).x;
    GH_CHECK_HIP(ctx, hipMemsetAsync(count, 0, (size_t)nkeys * 4, ctx->stream));  // (creation is not captured)
    hipLaunchKernelGGL(idg_count_kernel, dim3(g), dim3(256), 0, ctx->stream, p, count);
    hipLaunchKernelGGL(idg_scan_kernel, dim3(1), dim3(256), 0, ctx->stream, nkeys, count, offs, cursor, ioffs);
    hipLaunchKernelGGL(idg_bounds_kernel, dim3(1), dim3(256), 0, ctx->stream, L, nt2, offs, ioffs, bounds);
    hipLaunchKernelGGL(idg_scatter_kernel, dim3(g), dim3(256), 0, ctx->stream, p, cursor, cap, a, b, dw, src);
    GH_CHECK_HIP(ctx, hipGetLastError());
    std::vector<int32_t> hb((size_t)2 * (L + 1));
    GH_CHECK(d2h(ctx, hb.data(), bounds, hb.size() * 4));
    GH_CHECK(sync(ctx));
    const int64_t kept = hb[2 * L], nitems = hb[2 * L + 1];
    if (kept < 0 || kept > cap || nitems < 0) return fail(ctx, GRIDHIP_EHIP, "image-domain layers: the partition lost visibilities");
    for (int l = 0; l < L; ++l)
        slices->push_back(IdgSlice{hb[2 * l], hb[2 * l + 2] - hb[2 * l], hb[2 * l + 1], hb[2 * l + 3] - hb[2 * l + 1]});
    if (nitems == 0) return GRIDHIP_OK;
    void *q = nullptr;
    if (hipMalloc(&q, (size_t)nitems * sizeof(IdgItem)) != hipSuccess)
        return fail(ctx, GRIDHIP_ENOMEM, "image-domain layers: %lld work items", (long long)nitems);
    *items = (IdgItem *)q;  // (from here the caller frees it)
    GH_CHECK(scratch_prefill(ctx, q, (size_t)nitems * sizeof(IdgItem)));
    hipLaunchKernelGGL(idg_items_kernel, grid_for(ctx, nkeys), dim3(256), 0, ctx->stream, nkeys, (int)nt, Sg, K, count, offs, ioffs,
                       nitems, *items);
    GH_CHECK_HIP(ctx, hipGetLastError());
    return sync(ctx);  // (the tables go back to the pool)
}

int idg_grid(gridhip_ctx *ctx, int Sg, int K, int64_t N, double theta, const IdgItem *items, int64_t nitems, const double *a,
             const double *b, const double *dw, const double2 *vis, double2 *grid)
{
    if (nitems <= 0) return GRIDHIP_OK;
    const dim3 g((unsigned)nitems), blk(256);
    if (Sg == 16)
        hipLaunchKernelGGL(idg_grid_kernel<16>, g, blk, 0, ctx->stream, items, a, b, dw, vis, theta, K, N, (double *)grid);
    else if (Sg == 24)
        hipLaunchKernelGGL(idg_grid_kernel<24>, g, blk, 0, ctx->stream, items, a, b, dw, vis, theta, K, N, (double *)grid);
    else
        hipLaunchKernelGGL(idg_grid_kernel<32>, g, blk, 0, ctx->stream, items, a, b, dw, vis, theta, K, N, (double *)grid);
    GH_CHECK_HIP(ctx, hipGetLastError());
    return GRIDHIP_OK;
}

template <int SG>
static void idg_degrid_launch(gridhip_ctx *ctx, int K, int64_t N, double theta, const IdgItem *items, int64_t nitems, int64_t nvis,
                              const double *a, const double *b, const double *dw, const double2 *f, double2 *out)
{
    const dim3 g((unsigned)nitems);
    const int64_t mean = nvis / nitems;  // (the layer's, fixed at creation: the same launch every pass)
    if (mean <= 64)
        hipLaunchKernelGGL((idg_degrid_kernel<SG, 64>), g, dim3(64), 0, ctx->stream, items, a, b, dw, theta, K, N, f, out);
    else if (mean <= 128)
        hipLaunchKernelGGL((idg_degrid_kernel<SG, 128>), g, dim3(128), 0, ctx->stream, items, a, b, dw, theta, K, N, f, out);
    else
        hipLaunchKernelGGL((idg_degrid_kernel<SG, 256>), g, dim3(256), 0, ctx->stream, items, a, b, dw, theta, K, N, f, out);
}

int idg_degrid(gridhip_ctx *ctx, int Sg, int K, int64_t N, double theta, const IdgItem *items, int64_t nitems, int64_t nvis,
               const double *a, const double *b, const double *dw, const double2 *f, double2 *out)
{
    if (nitems <= 0) return GRIDHIP_OK;
    if (Sg == 16)
        idg_degrid_launch<16>(ctx, K, N, theta, items, nitems, nvis, a, b, dw, f, out);
    else if (Sg == 24)
        idg_degrid_launch<24>(ctx, K, N, theta, items, nitems, nvis, a, b, dw, f, out);
    else
        idg_degrid_launch<32>(ctx, K, N, theta, items, nitems, nvis, a, b, dw, f, out);
    GH_CHECK_HIP(ctx, hipGetLastError());
    return GRIDHIP_OK;
}

}  // namespace gridhip
