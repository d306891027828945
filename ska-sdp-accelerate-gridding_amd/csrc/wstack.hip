// W-stacking (include/gridhip.h, "w-stacking"): the w range of a stream cut into layers of M planes of `wstep`.  A layer is
// gridded by a gridhip_plan of its own with the w-projection kernels of the residual w alone - one table of M planes,
// K[r] = conj(w_kernel((r - M div 2) wstep)), for all layers - transformed to the image plane, multiplied there by the
// exact w-screen of its centre plane, S_l = exp(-2 pi i pc_l wstep (1 - sqrt(1 - l^2 - m^2))), and the layers are summed.
// The prediction is the exact adjoint: conj(S_l) x model, the forward transform, the gather with conj(K).
//
// The transforms run in place on the gridder's own N x N grid, without a roll pass either side.  With s = N div 2 and
// m = (N + 1) div 2 (the shifts of ishift2D and shift2D):
//   ifft_c(G)[y][x] = N^-2 exp(-2 pi i s (ky + kx) / N) B(G)[ky][kx],  k = (. + m) mod N,  B the unnormalised backward
//   transform of G as it lies - the input roll is a phase of the output (the shift theorem), the output roll an index;
//   fft_c(X)[k] = F(X')[k],  X'[j] = X[(j + s) mod N] exp(-2 pi i m (jy + jx) / N),  F the forward transform - the output
//   roll is a phase of the input.
// For even N both phases are the sign (-1)^(y + x); for odd N they are no sign, but the screen kernels form a phase per
// cell anyway and the shift's share is added to it in turns, reduced exactly in integers.
#include "common.h"
#include "imaging.h"
#include "idg.h"

namespace gridhip {

struct WsLayer {
    int64_t pc = 0;             // the centre plane pc_l
    int64_t off = 0, cnt = 0;   // its slice of the layer-ordered arrays
    gridhip_plan *plan = nullptr;
    int64_t ioff = 0, icnt = 0;  // image-domain layers: its slice of the work items (no plan)
};

}  // namespace gridhip

struct gridhip_wstack {
    gridhip_ctx *ctx = nullptr;
    double theta = 0.0;
    int64_t N = 0, n = 0, wstep = 0, M = 0;
    int64_t L = 0, pmin = 0, dropped = 0;
    std::vector<gridhip::WsLayer> layers;  // the occupied ones, by rising w
    bool clear_pred = false;               // some layer's gather leaves dropped visibilities unwritten
    bool grid_dirty = false;               // an image pass ended early: its grid is cleared before the next one
    // device memory of the stack's own (one block: base)
    void *base = nullptr;
    double *pu = nullptr, *pv = nullptr;   // u / lam, v / lam in layer order
    int64_t *rbin = nullptr;               // the residual bins r
    // image-domain layers (qpx == 0; idg.hip): Sg != 0, pu / pv / rbin hold a, b and the exact residual w (a double) in
    // (layer, tile) order, there is no table and no plan
    int Sg = 0, K = 0;
    gridhip::IdgItem *items = nullptr;     // the work items, a block of their own
    int32_t *src = nullptr;                // the visibility's index in the stream
    double2 *lay = nullptr;                // n values in layer order: the gathered vis of a grid pass, the predictions
    double2 *ktab = nullptr, *ktab_g = nullptr;  // K (the scatter's) and conj(K) (the gather's)
    double2 *grid = nullptr, *fgrid = nullptr;   // the scatter's grid (zero between passes) and the gather's
    void *fft = nullptr;                   // the handle's own transform; null: the context's cached one (the one-call forms)
    bool lent = false;                     // an imager's half stack: fft, ktab and ktab_g are the imager's (WsLend, imaging.h)
};

namespace gridhip {

namespace {

constexpr int WS_ITEMS = 8;  // visibilities per thread and chunk of the scatter pass

// (plane_of, finite_w and layer_of, the plane and layer rules, are in idg.h: the image-domain partition shares them)

// minimum and maximum plane over the finite w (ordered bits: imaging.h) and how many there are
__global__ void __launch_bounds__(256) ws_range_kernel(int64_t n, const double *__restrict__ w, int64_t stride, double wstep,
                                                       unsigned long long *__restrict__ out)
{
    unsigned long long mn = ~0ULL, mx = 0ULL, cnt = 0ULL;
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x) {
        const double x = w[k * stride];
        if (!finite_w(x)) continue;
        const unsigned long long b = ordered_bits(plane_of(x, wstep) + 0.0);  // (+ 0.0: no -0)
        mn = b < mn ? b : mn;
        mx = b > mx ? b : mx;
        ++cnt;
    }
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long a = __shfl_xor(mn, off, 64), b = __shfl_xor(mx, off, 64), c = __shfl_xor(cnt, off, 64);
        mn = a < mn ? a : mn;
        mx = b > mx ? b : mx;
        cnt += c;
    }
    __shared__ unsigned long long s[3][4];
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) s[0][wave] = mn, s[1][wave] = mx, s[2][wave] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < 4; ++i) {
            mn = s[0][i] < mn ? s[0][i] : mn;
            mx = s[1][i] > mx ? s[1][i] : mx;
            cnt += s[2][i];
        }
        if (cnt) {
            atomicMin(&out[0], mn);
            atomicMax(&out[1], mx);
            atomicAdd(&out[2], cnt);
        }
    }
}

// a[0 .. n) = value: tab[0 .. L] = 0 (the counts and the scan's total) before the counting pass; -1 in wstack_compose
__global__ void __launch_bounds__(256) ws_fill_i32_kernel(int64_t n, int32_t *__restrict__ a, int32_t value)
{
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x) a[k] = value;
}

// the counting pass: a histogram of the layers per work-group in LDS, added to count[L] at the end
__global__ void __launch_bounds__(256) ws_count_kernel(int64_t n, const double *__restrict__ w, int64_t stride, double wstep,
                                                       double pmin, int64_t M, int L, int32_t *__restrict__ count)
{
    extern __shared__ int32_t hist[];
    for (int l = threadIdx.x; l < L; l += blockDim.x) hist[l] = 0;
    __syncthreads();
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x) {
        int64_t r;
        const int l = layer_of(w[k * stride], wstep, pmin, M, &r);
        if (l >= 0 && l < L) atomicAdd(&hist[l], 1);
    }
    __syncthreads();
    for (int l = threadIdx.x; l < L; l += blockDim.x)
        if (hist[l]) atomicAdd(&count[l], hist[l]);
}

// offs[0 .. L] = the exclusive scan of count[0 .. L) and its total, cursor = offs: one work-group, 16 layers per thread
__global__ void __launch_bounds__(256) ws_scan_kernel(int L, const int32_t *__restrict__ count, int32_t *__restrict__ offs,
                                                      int32_t *__restrict__ cursor)
{
    __shared__ unsigned int lds[4];
    const int per = (L + 255) / 256, lo = threadIdx.x * per;
    unsigned int mine = 0;
    for (int i = lo; i < lo + per && i < L; ++i) mine += (unsigned int)count[i];
    unsigned int total;
    unsigned int run = block_rank(mine, lds, &total);
    for (int i = lo; i < lo + per && i < L; ++i) {
        offs[i] = (int32_t)run;
        cursor[i] = (int32_t)run;
        run += (unsigned int)count[i];
    }
    if (threadIdx.x == 0) offs[L] = (int32_t)total;
}

// The scatter pass: u / lam, v / lam, r and the stream index of every visibility with a layer into its layer's slice.  A
// work-group takes chunks of 256 x WS_ITEMS visibilities: ranks inside the chunk from an LDS histogram, one global add
// per layer and chunk for the chunk's place in the slice.  (The order inside a slice is the order the adds arrive in: it
// differs from run to run, as the order of the gridder's own records does.)
__global__ void __launch_bounds__(256) ws_scatter_kernel(int64_t n, const double *__restrict__ u, const double *__restrict__ v,
                                                         const double *__restrict__ w, int64_t stride, double lam,
                                                         double wstep, double pmin, int64_t M, int L,
                                                         int32_t *__restrict__ cursor, int64_t cap,
                                                         double *__restrict__ pu, double *__restrict__ pv,
                                                         int64_t *__restrict__ rbin, int32_t *__restrict__ src)
{
    extern __shared__ int32_t lds[];
    int32_t *cnt = lds, *first = lds + L;
    for (int l = threadIdx.x; l < L; l += blockDim.x) cnt[l] = 0;
    __syncthreads();
    const int64_t chunk = 256 * WS_ITEMS;
    for (int64_t c0 = (int64_t)blockIdx.x * chunk; c0 < n; c0 += (int64_t)gridDim.x * chunk) {
        int lay[WS_ITEMS], rank[WS_ITEMS];
        int64_t rr[WS_ITEMS];
#pragma unroll
        for (int i = 0; i < WS_ITEMS; ++i) {
            const int64_t k = c0 + i * 256 + threadIdx.x;
            lay[i] = -1;
            rr[i] = 0;
            rank[i] = 0;
            if (k < n) lay[i] = layer_of(w[k * stride], wstep, pmin, M, &rr[i]);
            if (lay[i] >= L) lay[i] = -1;
            if (lay[i] >= 0) rank[i] = atomicAdd(&cnt[lay[i]], 1);
        }
        __syncthreads();
        for (int l = threadIdx.x; l < L; l += blockDim.x) {
            const int32_t c = cnt[l];
            if (c) {
                first[l] = atomicAdd(&cursor[l], c);
                cnt[l] = 0;
            }
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < WS_ITEMS; ++i) {
            const int64_t k = c0 + i * 256 + threadIdx.x;
            if (lay[i] < 0) continue;
            const int64_t pos = (int64_t)first[lay[i]] + rank[i];
            if (pos < 0 || pos >= cap) continue;  // (cannot happen: the counts are of this very rule)
            pu[pos] = u[k * stride] / lam;
            pv[pos] = v[k * stride] / lam;
            rbin[pos] = rr[i];
            src[pos] = (int32_t)k;
        }
        // (the next chunk's ranks touch cnt only, and `first` is not written before its barrier)
    }
}

// lay[j] = vis[src[j]]: the permuting gather of a grid pass; *dropped_out = dropped (gridhip_last_dropped's counter)
__global__ void __launch_bounds__(256) ws_gather_kernel(int64_t m, const int32_t *__restrict__ src,
                                                        const double2 *__restrict__ vis, double2 *__restrict__ lay,
                                                        int32_t dropped, int32_t *__restrict__ dropped_out)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) *dropped_out = dropped;
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < m; j += (int64_t)gridDim.x * blockDim.x)
        lay[j] = vis[src[j]];
}

__global__ void __launch_bounds__(256) ws_zero_kernel(int64_t nd, double *__restrict__ a)
{
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < nd; k += (int64_t)gridDim.x * blockDim.x) a[k] = 0.0;
}

// c_i = (i - N div 2) / N theta; *ph = 1 - sqrt(1 - c_x^2 - c_y^2); false where c_x^2 + c_y^2 >= 1 (the factor 0)
__device__ __forceinline__ bool screen_ph(int64_t N, double theta, int64_t y, int64_t x, double *ph)
{
#pragma clang fp contract(off)
    const double cx = (double)(x - N / 2) / (double)N * theta, cy = (double)(y - N / 2) / (double)N * theta;
    const double r2 = cx * cx + cy * cy;
    *ph = 1.0 - sqrt(1.0 - r2);
    return r2 < 1.0;
}

// cos and sin of 2 pi (a + q / N) for a phase a in turns and integers 0 <= q < N: a is reduced to |.| <= 1/2 exactly
// (dft.hip's reduction), q / N is below 1
__device__ __forceinline__ void turns_sincos(double a, int64_t q, int64_t N, double *sn, double *cs)
{
    const double r = (a - rint(a)) + (double)q / (double)N;
    sincospi(2.0 * r, sn, cs);
}

// The tail of one layer of a grid pass.  h: the backward transform of the layer's grid, in place.  Per image cell: the
// transformed cell (the output roll is the index), times the input roll's phase and the screen S_l = exp(-2 pi i wc ph),
// its real part times `scale` added to the image (stored by the first layer), and a zero written back, so that the grid
// is clear for the next layer.  Every cell of h is read and cleared by exactly one thread.
// IDG (image-domain layers, margin K): the cell times the correction C[y][x] = c(y) c(x), and exactly 0 outside the
// trusted region; the w-projection stack's instantiations are as they were.
template <bool FIRST, bool IDG>
__global__ void __launch_bounds__(256) ws_screen_kernel(int64_t N, double theta, double wc, double2 *__restrict__ h,
                                                        double *__restrict__ image, double scale, int K)
{
    const int64_t cells = N * N, s = N / 2, m = (N + 1) / 2;
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < cells; c += (int64_t)gridDim.x * blockDim.x) {
        const int64_t y = c / N, x = c - y * N;
        int64_t ky = y + m, kx = x + m;
        ky -= ky >= N ? N : 0;
        kx -= kx >= N ? N : 0;
        const int64_t hc = ky * N + kx;
        const double2 z = h[hc];
        h[hc] = make_double2(0.0, 0.0);
        double ph, sn, cs, val = 0.0;
        if (screen_ph(N, theta, y, x, &ph)) {
            // turns: -wc ph - s (ky + kx) / N
            const int64_t q = (s * (ky + kx)) % N;
            turns_sincos(-(wc * ph), q == 0 ? 0 : N - q, N, &sn, &cs);
            val = scale * (z.x * cs - z.y * sn);
            if (IDG) {
                const double corr = idg_correction(y, N, K) * idg_correction(x, N, K);
                val = corr == 0.0 ? 0.0 : val * corr;
            }
        }
        image[c] = FIRST ? val : image[c] + val;
    }
}

// The head of one layer of a predict pass: f = X' of the file's head, X = conj(S_l) x model = model exp(+2 pi i wc ph), in
// the forward transform's input order, so that the transform's output is fft_c(X) as it lies.  IDG: X = conj(S_l) x C x
// model, and a cell outside the trusted region is not read.
template <bool IDG>
__global__ void __launch_bounds__(256) ws_head_kernel(int64_t N, double theta, double wc, const double *__restrict__ model,
                                                      double2 *__restrict__ f, int K)
{
    const int64_t cells = N * N, s = N / 2, m = (N + 1) / 2;
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < cells; c += (int64_t)gridDim.x * blockDim.x) {
        const int64_t jy = c / N, jx = c - jy * N;
        int64_t y = jy + s, x = jx + s;
        y -= y >= N ? N : 0;
        x -= x >= N ? N : 0;
        double ph, sn, cs;
        double2 out = make_double2(0.0, 0.0);
        if (screen_ph(N, theta, y, x, &ph)) {
            // turns: +wc ph - m (jy + jx) / N
            const int64_t q = (m * (jy + jx)) % N;
            turns_sincos(wc * ph, q == 0 ? 0 : N - q, N, &sn, &cs);
            if (IDG) {
                const double corr = idg_correction(y, N, K) * idg_correction(x, N, K);
                if (corr != 0.0) {
                    const double a = corr * model[y * N + x];
                    out = make_double2(a * cs, a * sn);
                }
            } else {
                const double a = model[y * N + x];
                out = make_double2(a * cs, a * sn);
            }
        }
        f[c] = out;
    }
}

// out[k] = 0, or sub[k], for every visibility (one without a layer predicts exactly 0), before the scatter below; sub may
// be out (then nothing is to do for the residual form, and the launcher skips this kernel)
__global__ void __launch_bounds__(256) ws_fill_kernel(int64_t n, const double2 *sub, double2 *out)
{
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x)
        out[k] = sub ? sub[k] : make_double2(0.0, 0.0);
}

// out[src[j]] = lay[j], or sub[src[j]] - lay[j]: the predictions back in stream order and the residual.  sub may be out:
// every index is read and written by one thread only.
__global__ void __launch_bounds__(256) ws_unpermute_kernel(int64_t m, const int32_t *__restrict__ src,
                                                           const double2 *__restrict__ lay, const double2 *sub, double2 *out,
                                                           int32_t dropped, int32_t *__restrict__ dropped_out)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) *dropped_out = dropped;
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < m; j += (int64_t)gridDim.x * blockDim.x) {
        const int64_t k = src[j];
        const double2 p = lay[j];
        if (sub) {
            const double2 a = sub[k];
            out[k] = make_double2(a.x - p.x, a.y - p.y);
        } else
            out[k] = p;
    }
}

// inv[src[j]] = j: the place in a stack's layer order of every visibility that has a layer
__global__ void __launch_bounds__(256) ws_invert_kernel(int64_t m, const int32_t *__restrict__ src, int32_t *__restrict__ inv)
{
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < m; j += (int64_t)gridDim.x * blockDim.x)
        inv[src[j]] = (int32_t)j;
}

// back[j'] = inv[src[j']]: where the other stack keeps the visibility that this one keeps at j'; *miss (when given) is
// set where the other stack does not keep it (inv = -1)
__global__ void __launch_bounds__(256) ws_compose_kernel(int64_t m, const int32_t *__restrict__ src,
                                                         const int32_t *__restrict__ inv, int32_t *__restrict__ back,
                                                         int32_t *__restrict__ miss)
{
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < m; j += (int64_t)gridDim.x * blockDim.x) {
        const int32_t i = inv[src[j]];
        back[j] = i;
        if (miss && i < 0) *miss = 1;
    }
}

// An imager's cycle middle (imager_middle_kernel, imager.hip) in the layer order of the mirrored stack, between the layers'
// gathers of the un-mirrored stack and the layers' scatters of the mirrored one: for the visibility k = src[j],
// r = vis[k] - layp[back[j]] (SUB) or vis[k]; vis_res[k] = r when asked; conj where sw[k] carries the sign, times |sw[k]|,
// into lay[j].  The expressions and their rounding are imager_middle_kernel's, so that vis_res has the same bits either way.
// vis_res may be vis: element k is read and written by the one lane that holds j.  A visibility without a layer is not
// visited (the launcher fills vis_res first).
template <bool SUB>
__global__ void __launch_bounds__(256)
    ws_middle_kernel(int64_t m, const int32_t *__restrict__ src, const int32_t *__restrict__ back, const double2 *vis,
                     const double2 *__restrict__ layp, const double *__restrict__ sw, double2 *__restrict__ lay,
                     double2 *vis_res, int32_t dropped, int32_t *__restrict__ dropped_out)
{
#pragma clang fp contract(off)
    if (blockIdx.x == 0 && threadIdx.x == 0) *dropped_out = dropped;
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < m; j += (int64_t)gridDim.x * blockDim.x) {
        const int64_t k = src[j];
        double2 r = vis[k];
        if (SUB) {
            const double2 p = layp[back[j]];
            r = make_double2(r.x - p.x, r.y - p.y);
        }
        if (vis_res) vis_res[k] = r;
        const double s = sw[k];
        const double a = fabs(s);
        if (signbit(s)) r.y = -r.y;
        lay[j] = a == 0.0 ? make_double2(0.0, 0.0) : make_double2(a * r.x, a * r.y);  // (selected out: vis may be NaN)
    }
}

// the maximum of x[0 .. cells) into *maxbits (ordered bits, initialised by the launcher): do_imaging's pmax
__global__ void __launch_bounds__(256) ws_max_kernel(int64_t cells, const double *__restrict__ x,
                                                     unsigned long long *__restrict__ maxbits)
{
    unsigned long long mx = 0ULL;
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < cells; c += (int64_t)gridDim.x * blockDim.x) {
        const unsigned long long b = ordered_bits(x[c]);
        mx = b > mx ? b : mx;
    }
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long b = __shfl_xor(mx, off, 64);
        mx = b > mx ? b : mx;
    }
    if ((threadIdx.x & 63) == 0) atomicMax(maxbits, mx);
}

size_t round16(size_t b) { return (b + 15) & ~(size_t)15; }

void wstack_free(gridhip_wstack *ws)
{
    if (!ws) return;
    for (WsLayer &l : ws->layers) gridhip_plan_destroy(l.plan);  // (synchronises the device)
    (void)hipSetDevice(ws->ctx->device);
    (void)hipDeviceSynchronize();
    if (!ws->lent) fft_plan_drop(ws->fft);
    if (ws->base) (void)hipFree(ws->base);
    if (ws->items) (void)hipFree(ws->items);
    delete ws;
}

}  // namespace

int wstack_check(gridhip_ctx *ctx, const WStackArgs &a, int64_t *N)
{
    *N = gridhip_image_size(a.theta, a.lam);
    // (qpx == 0: image-domain layers, npixKern the subgrid and npixFF the margin)
    const bool shape_ok = a.Q == 0 ? idg_shape_ok(a.S, a.npixFF) : w_kernel_shape_ok(a.npixFF, a.S, a.Q);
    if (*N <= 0 || a.wstep < 1 || a.M < 1 || !shape_ok || a.n < 0 || a.stride < 1 ||
        (a.n > 0 && (!a.u || !a.v || !a.w)))
        return fail(ctx, GRIDHIP_EINVAL, "w-stacking: bad argument (wstep, planes >= 1, the w-kernel shape rule or, with qpx 0, subgrid 16 / 24 / 32 and an even margin in [4, subgrid / 2], image size %lld)",
                    (long long)*N);
    if (a.n > (int64_t)0x7fffff00) return fail(ctx, GRIDHIP_EUNSUPPORTED, "n must be < 2^31 per stack");
    if (a.M > WS_MAX_PLANES) return fail(ctx, GRIDHIP_EUNSUPPORTED, "%lld planes per layer (at most 65536)", (long long)a.M);
    if (*N > 0x7fffffff) return fail(ctx, GRIDHIP_EUNSUPPORTED, "image size");
    return GRIDHIP_OK;
}

// the transform of a pass, bound to the context's stream
static int wstack_fft(gridhip_wstack *ws, void **plan)
{
    *plan = ws->fft;
    if (*plan) return fft_plan_bind(ws->ctx, *plan);
    return fft_plan_for(ws->ctx, ws->N, plan);
}

int wstack_tables(gridhip_ctx *ctx, const WStackArgs &a, double2 *ktab, double2 *ktab_g)
{
    if (a.Q == 0) return GRIDHIP_OK;  // image-domain layers have no table
    GH_CHECK(build_w_planes(ctx, a.theta, a.wstep, -(a.M / 2) * a.wstep, a.M, a.npixFF, a.S, a.Q, ktab, true));
    return launch_conj_copy(ctx, a.M * a.Q * a.Q * a.S * a.S, ktab, ktab_g);
}

static int wstack_build(gridhip_ctx *ctx, const WStackArgs &a, int64_t N, bool own_fft, const WsLend *lend, gridhip_wstack *ws)
{
    const int64_t n = a.n;
    ws->ctx = ctx, ws->theta = a.theta, ws->N = N, ws->n = n, ws->wstep = a.wstep, ws->M = a.M;
    const bool idg = a.Q == 0;
    if (idg) ws->Sg = (int)a.S, ws->K = (int)a.npixFF;
    // ---- the plane range of the finite w, back to the host (as the w-bin rule of w_cache_imaging reads its own back)
    unsigned long long range[3] = {~0ULL, 0ULL, 0ULL};
    if (n > 0) {
        DevBuf dr;
        GH_CHECK(dr.upload(ctx, range, sizeof range));
        unsigned g = grid_for(ctx, n).x;
        if (g > (unsigned)ctx->num_cu * 4) g = (unsigned)ctx->num_cu * 4;
        hipLaunchKernelGGL(ws_range_kernel, dim3(g), dim3(256), 0, ctx->stream, n, a.w, a.stride, (double)a.wstep,
                           dr.as<unsigned long long>());
        GH_CHECK_HIP(ctx, hipGetLastError());
        GH_CHECK(d2h(ctx, range, dr.p, sizeof range));
        GH_CHECK(sync(ctx));
    }
    const int64_t nfinite = (int64_t)range[2];
    ws->dropped = n - nfinite;
    double pmin = 0.0;
    if (nfinite > 0) {
        pmin = ordered_value(range[0]);
        const double pmax = ordered_value(range[1]);
        if (!(fabs(pmin) <= 4503599627370496.0 && fabs(pmax) <= 4503599627370496.0))
            return fail(ctx, GRIDHIP_EUNSUPPORTED, "w-stacking: |w / wstep| above 2^52");
        const double layers = floor((pmax - pmin) / (double)a.M) + 1.0;
        if (layers > (double)WS_MAX_LAYERS)
            return fail(ctx, GRIDHIP_EUNSUPPORTED, "w-stacking: %.0f layers (at most 4096): raise planes or wstep", layers);
        ws->pmin = (int64_t)pmin;
        ws->L = ((int64_t)pmax - (int64_t)pmin) / a.M + 1;
    }
    const int L = (int)ws->L;
    // ---- the stack's own memory, one block
    const size_t cells = (size_t)N * N, tab = (size_t)a.M * a.Q * a.Q * a.S * a.S;
    // (an imager's half stack: the tables are the imager's, and of the two grids it has the one its passes use)
    const bool own_tab = !lend, own_grid = !lend || lend->half == 2, own_fgrid = !lend || lend->half == 1;
    const size_t sizes[] = {(size_t)nfinite * 8, (size_t)nfinite * 8, (size_t)nfinite * 8, (size_t)nfinite * 4,
                            (size_t)nfinite * 16, own_tab ? tab * 16 : 0, own_tab ? tab * 16 : 0, own_grid ? cells * 16 : 0,
                            own_fgrid ? cells * 16 : 0};
    size_t total = 0, at[9];
    for (int i = 0; i < 9; ++i) {
        at[i] = total;
        total += round16(sizes[i]) + 256;
    }
    if (hipMalloc(&ws->base, total) != hipSuccess) {
        ws->base = nullptr;
        return fail(ctx, GRIDHIP_ENOMEM, "w-stacking: %zu bytes", total);
    }
    GH_CHECK(scratch_prefill(ctx, ws->base, total));
    char *b = (char *)ws->base;
    ws->pu = (double *)(b + at[0]), ws->pv = (double *)(b + at[1]), ws->rbin = (int64_t *)(b + at[2]);
    ws->src = (int32_t *)(b + at[3]), ws->lay = (double2 *)(b + at[4]);
    ws->ktab = (double2 *)(b + at[5]), ws->ktab_g = (double2 *)(b + at[6]);
    ws->grid = own_grid ? (double2 *)(b + at[7]) : nullptr, ws->fgrid = own_fgrid ? (double2 *)(b + at[8]) : nullptr;
    if (lend) ws->lent = true, ws->fft = lend->fft, ws->ktab = lend->ktab, ws->ktab_g = lend->ktab_g;
    if (own_grid)
        hipLaunchKernelGGL(ws_zero_kernel, grid_for(ctx, (int64_t)cells), dim3(256), 0, ctx->stream, (int64_t)cells * 2,
                           (double *)ws->grid);
    GH_CHECK_HIP(ctx, hipGetLastError());
    // (making a hipFFT plan loads its kernels: about 16 ms at N = 2048, as much again to drop it - a handle pays it once,
    // the one-call forms take the context's cached plan, as kind 2 does)
    if (own_fft && !lend) GH_CHECK(fft_plan_own(ctx, N, &ws->fft));
    if (L == 0) return GRIDHIP_OK;
    if (idg) {
        // ---- image-domain layers: the partition by (layer, tile), a, b and the exact residual w in place of pu, pv and r
        std::vector<IdgSlice> slices;
        GH_CHECK(idg_partition(ctx, a, N, pmin, L, nfinite, ws->pu, ws->pv, (double *)ws->rbin, ws->src, &slices, &ws->items));
        int64_t kept = 0;
        for (int l = 0; l < L; ++l) {
            kept += slices[l].cnt;
            if (slices[l].cnt <= 0) continue;
            WsLayer lay;
            lay.pc = ws->pmin + (int64_t)l * a.M + a.M / 2;
            lay.off = slices[l].off, lay.cnt = slices[l].cnt, lay.ioff = slices[l].ioff, lay.icnt = slices[l].icnt;
            ws->layers.push_back(lay);
        }
        ws->dropped = n - kept;  // (outside the grid, or NaN in u or v: with those without a finite w)
        return GRIDHIP_OK;
    }
    // ---- the layer partition: count, scan, scatter; the slices' bounds back to the host
    DevBuf dtab;  // count[L], offs[L + 1], cursor[L]
    GH_CHECK(dtab.alloc(ctx, (size_t)(3 * L + 1) * 4));
    int32_t *count = dtab.as<int32_t>(), *offs = count + L, *cursor = offs + L + 1;
    hipLaunchKernelGGL(ws_fill_i32_kernel, dim3(1), dim3(256), 0, ctx->stream, (int64_t)(3 * L + 1), count, 0);
    unsigned gc = grid_for(ctx, n).x;  // (every work-group ends with up to L global adds: few, long ones)
    if (gc > (unsigned)ctx->num_cu * 4) gc = (unsigned)ctx->num_cu * 4;
    hipLaunchKernelGGL(ws_count_kernel, dim3(gc), dim3(256), (size_t)L * 4, ctx->stream, n, a.w, a.stride, (double)a.wstep,
                       pmin, a.M, L, count);
    hipLaunchKernelGGL(ws_scan_kernel, dim3(1), dim3(256), 0, ctx->stream, L, count, offs, cursor);
    hipLaunchKernelGGL(ws_scatter_kernel, grid_for(ctx, (n + WS_ITEMS - 1) / WS_ITEMS), dim3(256), (size_t)L * 8, ctx->stream,
                       n, a.u, a.v, a.w, a.stride, (double)a.lam, (double)a.wstep, pmin, a.M, L, cursor, nfinite, ws->pu,
                       ws->pv, ws->rbin, ws->src);
    GH_CHECK_HIP(ctx, hipGetLastError());
    std::vector<int32_t> hoffs((size_t)L + 1);
    GH_CHECK(d2h(ctx, hoffs.data(), offs, hoffs.size() * 4));
    // ---- the kernel table of the residual planes, and its conjugate for the gather
    if (own_tab) GH_CHECK(wstack_tables(ctx, a, ws->ktab, ws->ktab_g));
    GH_CHECK(sync(ctx));
    if (hoffs[L] != nfinite) return fail(ctx, GRIDHIP_EHIP, "w-stacking: the partition lost visibilities");
    // ---- one plan per occupied layer over its slice
    for (int l = 0; l < L; ++l) {
        const int64_t off = hoffs[l], cnt = hoffs[l + 1] - hoffs[l];
        if (cnt <= 0) continue;
        WsLayer lay;
        lay.pc = ws->pmin + (int64_t)l * a.M + a.M / 2;
        lay.off = off, lay.cnt = cnt;
        GH_CHECK(gridhip_plan_create_dev(ctx, N, N, cnt, a.M, a.Q, a.S, a.S, ws->pu + off, ws->pv + off, 1, ws->rbin + off,
                                         &lay.plan));
        ws->layers.push_back(lay);  // (from here the stack destroys the plan)
        int64_t d = 0;
        GH_CHECK(gridhip_last_dropped(ctx, &d));
        ws->dropped += d;
        if (plan_caller_clears(lay.plan)) ws->clear_pred = true;
    }
    return GRIDHIP_OK;
}

int wstack_create(gridhip_ctx *ctx, const WStackArgs &a, int64_t N, gridhip_wstack **out, bool own_fft, const WsLend *lend)
{
    *out = nullptr;
    GH_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    gridhip_wstack *ws = new (std::nothrow) gridhip_wstack();
    if (!ws) return GRIDHIP_ENOMEM;
    ws->ctx = ctx;
    int rc = wstack_build(ctx, a, N, own_fft, lend, ws);
    if (rc == GRIDHIP_OK) {
        // gridhip_last_dropped reports the whole stack, not its last layer's plan
        const int32_t d = (int32_t)ws->dropped;
        rc = h2d(ctx, ctx->d_scalars, &d, sizeof d);
        if (rc == GRIDHIP_OK) rc = sync(ctx);
    }
    if (rc != GRIDHIP_OK) {
        const std::string msg = ctx->err;  // (freeing may not lose the reason)
        wstack_free(ws);
        ctx->err = msg;
        return rc;
    }
    *out = ws;
    return GRIDHIP_OK;
}

int64_t wstack_count(const gridhip_wstack *ws) { return ws->layers.empty() ? 0 : ws->layers.back().off + ws->layers.back().cnt; }

int wstack_image_run(gridhip_wstack *ws, const double *vis, double *image, double factor)
{
    gridhip_ctx *ctx = ws->ctx;
    const int64_t m = wstack_count(ws);
    if (m > 0) {
        hipLaunchKernelGGL(ws_gather_kernel, grid_for(ctx, m), dim3(256), 0, ctx->stream, m, ws->src, (const double2 *)vis,
                           ws->lay, (int32_t)ws->dropped, ctx->d_scalars);
        GH_CHECK_HIP(ctx, hipGetLastError());
    }
    return wstack_image_layers(ws, image, factor);
}

int wstack_image_layers(gridhip_wstack *ws, double *image, double factor)
{
    gridhip_ctx *ctx = ws->ctx;
    const int64_t N = ws->N, cells = N * N;
    if (ws->layers.empty()) {
        hipLaunchKernelGGL(ws_zero_kernel, grid_for(ctx, cells), dim3(256), 0, ctx->stream, cells, image);
        GH_CHECK_HIP(ctx, hipGetLastError());
        return GRIDHIP_OK;
    }
    if (ws->grid_dirty)
        hipLaunchKernelGGL(ws_zero_kernel, grid_for(ctx, cells), dim3(256), 0, ctx->stream, cells * 2, (double *)ws->grid);
    ws->grid_dirty = true;
    void *fft = nullptr;
    GH_CHECK(wstack_fft(ws, &fft));
    const double scale = factor / ((double)N * (double)N);
    bool first = true;
    for (const WsLayer &l : ws->layers) {
        if (ws->Sg)
            GH_CHECK(idg_grid(ctx, ws->Sg, ws->K, N, ws->theta, ws->items + l.ioff, l.icnt, ws->pu, ws->pv,
                              (const double *)ws->rbin, ws->lay, ws->grid));
        else
            GH_CHECK(gridhip_plan_grid_dev(l.plan, (const double *)ws->ktab, (const double *)(ws->lay + l.off),
                                           (double *)ws->grid));
        GH_CHECK(fft_exec(ctx, fft, ws->grid, true));
        const double wc = (double)l.pc * (double)ws->wstep;
        auto screen = ws->Sg ? (first ? ws_screen_kernel<true, true> : ws_screen_kernel<false, true>)
                             : (first ? ws_screen_kernel<true, false> : ws_screen_kernel<false, false>);
        hipLaunchKernelGGL(screen, grid_for(ctx, cells), dim3(256), 0, ctx->stream, N, ws->theta, wc, ws->grid, image, scale,
                           ws->K);
        GH_CHECK_HIP(ctx, hipGetLastError());
        first = false;
    }
    ws->grid_dirty = false;
    return GRIDHIP_OK;
}

int wstack_predict_run(gridhip_wstack *ws, const double *model, const double *vis_sub, double *vis_out)
{
    gridhip_ctx *ctx = ws->ctx;
    const int64_t n = ws->n;
    if (n == 0) return GRIDHIP_OK;
    const double2 *sub = (const double2 *)vis_sub;
    double2 *out = (double2 *)vis_out;
    // a visibility without a layer: 0, or vis_sub[k] (in place: it is there already)
    const int64_t m = wstack_count(ws);
    if (m < n && sub != out) hipLaunchKernelGGL(ws_fill_kernel, grid_for(ctx, n), dim3(256), 0, ctx->stream, n, sub, out);
    GH_CHECK_HIP(ctx, hipGetLastError());
    if (m == 0) return GRIDHIP_OK;
    GH_CHECK(wstack_predict_layers(ws, model));
    hipLaunchKernelGGL(ws_unpermute_kernel, grid_for(ctx, m), dim3(256), 0, ctx->stream, m, ws->src, ws->lay, sub, out,
                       (int32_t)ws->dropped, ctx->d_scalars);
    GH_CHECK_HIP(ctx, hipGetLastError());
    return GRIDHIP_OK;
}

int wstack_predict_layers(gridhip_wstack *ws, const double *model)
{
    gridhip_ctx *ctx = ws->ctx;
    const int64_t N = ws->N, cells = N * N, m = wstack_count(ws);
    if (m == 0) return GRIDHIP_OK;
    if (ws->clear_pred)
        hipLaunchKernelGGL(ws_zero_kernel, grid_for(ctx, m), dim3(256), 0, ctx->stream, m * 2, (double *)ws->lay);
    void *fft = nullptr;
    GH_CHECK(wstack_fft(ws, &fft));
    for (const WsLayer &l : ws->layers) {
        hipLaunchKernelGGL(ws->Sg ? ws_head_kernel<true> : ws_head_kernel<false>, grid_for(ctx, cells), dim3(256), 0, ctx->stream,
                           N, ws->theta, (double)l.pc * (double)ws->wstep, model, ws->fgrid, ws->K);
        GH_CHECK_HIP(ctx, hipGetLastError());
        GH_CHECK(fft_exec(ctx, fft, ws->fgrid, false));
        if (ws->Sg)
            GH_CHECK(idg_degrid(ctx, ws->Sg, ws->K, N, ws->theta, ws->items + l.ioff, l.icnt, l.cnt, ws->pu, ws->pv,
                                (const double *)ws->rbin, ws->fgrid, ws->lay));
        else
            GH_CHECK(gridhip_plan_degrid_dev(l.plan, (const double *)ws->ktab_g, (const double *)ws->fgrid,
                                             (double *)(ws->lay + l.off)));
    }
    return GRIDHIP_OK;
}

int wstack_compose(gridhip_wstack *from, gridhip_wstack *to, int32_t *back, bool *same)
{
    gridhip_ctx *ctx = to->ctx;
    const int64_t m = wstack_count(to);
    *same = true;
    // Image-domain layers drop a visibility that lies off the grid, and 0 <= x < N is not symmetric under the mirror (x = 0
    // against x = N; an odd N): the two stacks may keep different visibilities, which is found here and is no error.
    const bool idg = to->Sg != 0;
    if (wstack_count(from) != m || from->n != to->n) {
        if (!idg) return fail(ctx, GRIDHIP_EHIP, "w-stacking: the two streams of an imager differ in their finite w");
        *same = false;
        return GRIDHIP_OK;
    }
    if (m == 0) return GRIDHIP_OK;
    // (w-projection: every entry that is read has been written, the two stacks hold the same visibilities; image-domain
    // layers: inv starts at -1, and its last entry is set when `to` keeps a visibility that `from` does not)
    DevBuf inv;
    GH_CHECK(inv.alloc(ctx, (size_t)(to->n + 1) * 4));
    int32_t *miss = idg ? inv.as<int32_t>() + to->n : nullptr;
    if (idg) {
        hipLaunchKernelGGL(ws_fill_i32_kernel, grid_for(ctx, to->n), dim3(256), 0, ctx->stream, to->n, inv.as<int32_t>(), -1);
        hipLaunchKernelGGL(ws_fill_i32_kernel, dim3(1), dim3(256), 0, ctx->stream, (int64_t)1, miss, 0);
    }
    hipLaunchKernelGGL(ws_invert_kernel, grid_for(ctx, m), dim3(256), 0, ctx->stream, m, from->src, inv.as<int32_t>());
    hipLaunchKernelGGL(ws_compose_kernel, grid_for(ctx, m), dim3(256), 0, ctx->stream, m, to->src, inv.as<int32_t>(), back, miss);
    GH_CHECK_HIP(ctx, hipGetLastError());
    if (idg) {
        int32_t h = 0;
        GH_CHECK(d2h(ctx, &h, miss, 4));
        GH_CHECK(sync(ctx));
        *same = h == 0;
    }
    return GRIDHIP_OK;
}

int wstack_middle_run(gridhip_wstack *from, gridhip_wstack *to, const int32_t *back, const double *vis, const double *sw,
                      double *vis_res)
{
    gridhip_ctx *ctx = to->ctx;
    const int64_t n = to->n, m = wstack_count(to);
    const double2 *v = (const double2 *)vis;
    double2 *res = (double2 *)vis_res;
    // a visibility without a layer is not visited: its residual is vis[k] (in place: it is there already)
    if (m < n && res && res != v) hipLaunchKernelGGL(ws_fill_kernel, grid_for(ctx, n), dim3(256), 0, ctx->stream, n, v, res);
    if (m > 0) {
        if (from)
            hipLaunchKernelGGL(ws_middle_kernel<true>, grid_for(ctx, m), dim3(256), 0, ctx->stream, m, to->src, back, v,
                               (const double2 *)from->lay, sw, to->lay, res, (int32_t)to->dropped, ctx->d_scalars);
        else
            hipLaunchKernelGGL(ws_middle_kernel<false>, grid_for(ctx, m), dim3(256), 0, ctx->stream, m, to->src, back, v,
                               (const double2 *)nullptr, sw, to->lay, res, (int32_t)to->dropped, ctx->d_scalars);
    }
    GH_CHECK_HIP(ctx, hipGetLastError());
    return GRIDHIP_OK;
}

int wstack_image_max(gridhip_ctx *ctx, int64_t cells, const double *x, unsigned long long *maxbits)
{
    static const unsigned long long neg_inf_bits = ordered_bits(-INFINITY);  // (static: the source of an async copy)
    GH_CHECK(h2d(ctx, maxbits, &neg_inf_bits, 8));
    hipLaunchKernelGGL(ws_max_kernel, dim3((unsigned)ctx->num_cu * 4), dim3(256), 0, ctx->stream, cells, x, maxbits);
    GH_CHECK_HIP(ctx, hipGetLastError());
    return GRIDHIP_OK;
}

void wstack_release(gridhip_wstack *ws) { wstack_free(ws); }

namespace {

// do_imaging with a stack (include/gridhip.h): mirror, doweight on the mirrored u, v, one stack on the mirrored stream,
// image = 2 Re D(wt vis1), psf = 2 Re D(wt), both divided by the PSF's maximum
int do_imaging_wstack_any(gridhip_ctx *ctx, bool dev, WStackArgs a, const double *vis, double *image, double *psf, double *pmax)
{
    if (!ctx) return GRIDHIP_EINVAL;
    int64_t N = 0;
    GH_CHECK(wstack_check(ctx, a, &N));
    if (!image || !psf || (a.n > 0 && !vis)) return fail(ctx, GRIDHIP_EINVAL, "bad argument");
    GH_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    const int64_t n = a.n;
    const size_t cells = (size_t)N * N, span = span_bytes(n, a.stride);
    Staged st(ctx, dev);
    const double *u = st.in(a.u, span), *v = st.in(a.v, span), *w = st.in(a.w, span);
    vis = st.in(vis, (size_t)n * 16);
    image = st.out(image, cells * 8), psf = st.out(psf, cells * 8);
    GH_CHECK(st.status());
    static const unsigned long long neg_inf_bits = ordered_bits(-INFINITY);  // (static: the source of an async copy)
    DevBuf du, dv, dw, dvis, dwt, dpu, dpv, dcnt, dmax;
    GH_CHECK(dvis.alloc(ctx, (size_t)n * 16));
    GH_CHECK(dwt.alloc(ctx, (size_t)n * 16));
    GH_CHECK(dcnt.alloc(ctx, cells * 4));
    GH_CHECK(dmax.upload(ctx, &neg_inf_bits, 8));
    GH_CHECK(slice_uvw(ctx, n, u, v, w, a.stride, du, dv, dw));
    GH_CHECK(copy_in(ctx, dvis.p, vis, (size_t)n * 16, true));
    GH_CHECK(launch_mirror(ctx, n, du.as<double>(), dv.as<double>(), dw.as<double>(), dvis.as<double2>()));
    GH_CHECK(scaled_uv(ctx, n, du.as<double>(), dv.as<double>(), 1, (double)a.lam, dpu, dpv));
    if (n > 0) {
        GH_CHECK(launch_fill_ones(ctx, n, dwt.as<double2>()));
        GH_CHECK_HIP(ctx, hipMemsetAsync(dcnt.p, 0, cells * 4, ctx->stream));
        GH_CHECK(launch_doweight(ctx, N, n, dpu.as<double>(), dpv.as<double>(), dcnt.as<unsigned int>(), dwt.as<double2>()));
        GH_CHECK(launch_cmul(ctx, n, dwt.as<double2>(), dvis.as<double2>(), dvis.as<double2>()));
    }
    a.u = du.as<double>(), a.v = dv.as<double>(), a.w = dw.as<double>(), a.stride = 1;
    gridhip_wstack *ws = nullptr;
    GH_CHECK(wstack_create(ctx, a, N, &ws, false));
    int rc = wstack_image_run(ws, dvis.as<double>(), image, 2.0);
    if (rc == GRIDHIP_OK) rc = wstack_image_run(ws, dwt.as<double>(), psf, 2.0);
    if (rc == GRIDHIP_OK) {
        hipLaunchKernelGGL(ws_max_kernel, dim3((unsigned)ctx->num_cu * 4), dim3(256), 0, ctx->stream, (int64_t)cells, psf,
                           dmax.as<unsigned long long>());
        rc = normalise(ctx, cells, image, psf, dmax.as<unsigned long long>(), pmax);  // (synchronises)
    }
    const std::string msg = ctx->err;
    wstack_free(ws);
    ctx->err = msg;
    GH_CHECK(rc);
    return st.finish();
}

int predict_wstack_any(gridhip_ctx *ctx, bool dev, const WStackArgs &a, const double *model, const double *vis_sub,
                       double *vis_out)
{
    if (!ctx) return GRIDHIP_EINVAL;
    int64_t N = 0;
    GH_CHECK(wstack_check(ctx, a, &N));
    if (!model || (a.n > 0 && !vis_out)) return fail(ctx, GRIDHIP_EINVAL, "bad argument");
    GH_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    const int64_t n = a.n;
    GH_CHECK_HIP(ctx, hipMemsetAsync(ctx->d_scalars, 0, 4 * sizeof(int32_t), ctx->stream));  // nothing dropped so far
    Staged st(ctx, dev);
    if (n == 0) return st.finish();
    const size_t span = span_bytes(n, a.stride);
    WStackArgs d = a;
    model = st.in(model, (size_t)N * N * 8);
    d.u = st.in(a.u, span), d.v = st.in(a.v, span), d.w = st.in(a.w, span);
    vis_sub = st.in(vis_sub, (size_t)n * 16);
    vis_out = st.out(vis_out, (size_t)n * 16);
    GH_CHECK(st.status());
    gridhip_wstack *ws = nullptr;
    GH_CHECK(wstack_create(ctx, d, N, &ws, false));
    int rc = wstack_predict_run(ws, model, vis_sub, vis_out);
    if (rc == GRIDHIP_OK) rc = sync(ctx);
    const std::string msg = ctx->err;
    wstack_free(ws);
    ctx->err = msg;
    GH_CHECK(rc);
    return st.finish();
}

}  // namespace
}  // namespace gridhip

using namespace gridhip;

extern "C" {

int gridhip_wstack_create_dev(gridhip_ctx *ctx, int64_t wstep, int64_t M, int64_t qpx, int64_t npixFF, int64_t npixKern,
                              double theta, int64_t lam, int64_t n, const double *u, const double *v, const double *w,
                              int64_t uv_stride, gridhip_wstack **ws)
{
    if (!ctx || !ws) return GRIDHIP_EINVAL;
    *ws = nullptr;
    const WStackArgs a{wstep, M, qpx, npixFF, npixKern, theta, lam, n, u, v, w, uv_stride};
    int64_t N = 0;
    GH_CHECK(wstack_check(ctx, a, &N));
    return wstack_create(ctx, a, N, ws);
}

int gridhip_wstack_image_dev(gridhip_wstack *ws, const double *vis, double *image)
{
    if (!ws) return GRIDHIP_EINVAL;
    if (!image || (ws->n > 0 && !vis)) return fail(ws->ctx, GRIDHIP_EINVAL, "null pointer");
    GH_CHECK_HIP(ws->ctx, hipSetDevice(ws->ctx->device));
    return wstack_image_run(ws, vis, image, 1.0);
}

int gridhip_wstack_predict_dev(gridhip_wstack *ws, const double *model, const double *vis_sub, double *vis_out)
{
    if (!ws) return GRIDHIP_EINVAL;
    if (!model || (ws->n > 0 && !vis_out)) return fail(ws->ctx, GRIDHIP_EINVAL, "null pointer");
    GH_CHECK_HIP(ws->ctx, hipSetDevice(ws->ctx->device));
    return wstack_predict_run(ws, model, vis_sub, vis_out);
}

int gridhip_wstack_info(gridhip_wstack *ws, int64_t *layers, int64_t *occupied, int64_t *pmin, int64_t *dropped)
{
    if (!ws) return GRIDHIP_EINVAL;
    if (layers) *layers = ws->L;
    if (occupied) *occupied = (int64_t)ws->layers.size();
    if (pmin) *pmin = ws->pmin;
    if (dropped) *dropped = ws->dropped;
    return GRIDHIP_OK;
}

int gridhip_wstack_destroy(gridhip_wstack *ws)
{
    wstack_free(ws);
    return GRIDHIP_OK;
}

int gridhip_do_imaging_wstack(gridhip_ctx *ctx, int64_t wstep, int64_t M, int64_t qpx, int64_t npixFF, int64_t npixKern,
                              double theta, int64_t lam, int64_t n, const double *u, const double *v, const double *w,
                              int64_t uv_stride, const double *vis, double *image, double *psf, double *pmax)
{
    return do_imaging_wstack_any(ctx, false, {wstep, M, qpx, npixFF, npixKern, theta, lam, n, u, v, w, uv_stride}, vis, image,
                                 psf, pmax);
}

int gridhip_do_imaging_wstack_dev(gridhip_ctx *ctx, int64_t wstep, int64_t M, int64_t qpx, int64_t npixFF, int64_t npixKern,
                                  double theta, int64_t lam, int64_t n, const double *u, const double *v, const double *w,
                                  int64_t uv_stride, const double *vis, double *image, double *psf, double *pmax)
{
    return do_imaging_wstack_any(ctx, true, {wstep, M, qpx, npixFF, npixKern, theta, lam, n, u, v, w, uv_stride}, vis, image,
                                 psf, pmax);
}

int gridhip_predict_wstack(gridhip_ctx *ctx, int64_t wstep, int64_t M, int64_t qpx, int64_t npixFF, int64_t npixKern,
                           double theta, int64_t lam, const double *model, int64_t n, const double *u, const double *v,
                           const double *w, int64_t uv_stride, const double *vis_sub, double *vis_out)
{
    return predict_wstack_any(ctx, false, {wstep, M, qpx, npixFF, npixKern, theta, lam, n, u, v, w, uv_stride}, model, vis_sub,
                              vis_out);
}

int gridhip_predict_wstack_dev(gridhip_ctx *ctx, int64_t wstep, int64_t M, int64_t qpx, int64_t npixFF, int64_t npixKern,
                               double theta, int64_t lam, const double *model, int64_t n, const double *u, const double *v,
                               const double *w, int64_t uv_stride, const double *vis_sub, double *vis_out)
{
    return predict_wstack_any(ctx, true, {wstep, M, qpx, npixFF, npixKern, theta, lam, n, u, v, w, uv_stride}, model, vis_sub,
                              vis_out);
}

}  // extern "C"
