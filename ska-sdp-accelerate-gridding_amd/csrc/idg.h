// Image-domain layers of a w-stack (include/gridhip.h, "w-stacking", IMAGE-DOMAIN LAYERS; idg.hip): what wstack.hip needs
// of them.  A stack made with qpx == 0 forms a layer's grid from subgrids: the visibilities of one uv tile are summed as a
// direct Fourier sum onto an Sg x Sg image with their exact residual w, tapered, transformed and added to the grid.
#pragma once
#include "common.h"
#include "imaging.h"

namespace gridhip {

constexpr int IDG_CHUNK = 256;   // read-only option "idg_chunk": the visibilities a work-group stages in LDS at a time
constexpr int IDG_SPLIT = 1024;  // read-only option "idg_split": a tile with more visibilities is cut into work items of this many
constexpr int64_t IDG_MAX_KEYS = (int64_t)1 << 26;  // layers x tiles of a stack: four 32-bit tables of that many entries

// the subgrid Sg and the margin K of a stack with qpx == 0 (npixKern and npixFF)
static inline bool idg_shape_ok(int64_t Sg, int64_t K)
{
    return (Sg == 16 || Sg == 24 || Sg == 32) && K % 2 == 0 && K >= 4 && K <= Sg / 2;
}

// one work item: the subgrid's origin cell, and its slice of the tile-ordered arrays (a whole tile, or a piece of a split one)
struct IdgItem {
    int32_t ox, oy, off, cnt;
};

// the slice of one layer in the tile-ordered arrays and in the item list
struct IdgSlice {
    int64_t off, cnt, ioff, icnt;
};

// The plane of a finite w: libm round, as the w-bin rule (wround_kernel, image_ops.hip)
__device__ __forceinline__ double plane_of(double w, double wstep) { return round(w / wstep); }
__device__ __forceinline__ bool finite_w(double w) { return fabs(w) < __builtin_inf(); }

// The layer of visibility k, or -1 without a finite w; *r: its residual bin.  pmin and M are exact in doubles (the host
// has checked |plane| <= 2^52), and (p - pmin) / M is below L <= 4096.
__device__ __forceinline__ int layer_of(double w, double wstep, double pmin, int64_t M, int64_t *r)
{
    if (!finite_w(w)) return -1;
    const int64_t d = (int64_t)(plane_of(w, wstep) - pmin);
    const int64_t l = d / M;
    *r = d - l * M;
    return (int)l;
}

// The partition of a stream by (layer, tile): a[j], b[j], dw[j] and the stream index src[j] of every kept visibility, layer
// by layer and tile by tile inside a layer (the order inside a tile is the order the adds arrive in), slices[l] for every
// layer 0 .. L - 1, and the work items in *items (one device block of the stack's own, hipFree'd by the caller).
// cap: the room of a, b, dw, src.  Synchronises.
int idg_partition(gridhip_ctx *ctx, const WStackArgs &args, int64_t N, double pmin, int L, int64_t cap, double *a, double *b,
                  double *dw, int32_t *src, std::vector<IdgSlice> *slices, IdgItem **items);

// grid += the subgrids of `nitems` work items of one layer (vis in the partition's order); kernels only
int idg_grid(gridhip_ctx *ctx, int Sg, int K, int64_t N, double theta, const IdgItem *items, int64_t nitems, const double *a,
             const double *b, const double *dw, const double2 *vis, double2 *grid);
// out[j] = the prediction of every visibility of the items (nvis in all: it sizes the work-groups) from
// f = fft_c(conj(S_l) x C x model); kernels only, no atomics
int idg_degrid(gridhip_ctx *ctx, int Sg, int K, int64_t N, double theta, const IdgItem *items, int64_t nitems, int64_t nvis,
               const double *a, const double *b, const double *dw, const double2 *f, double2 *out);

// c(x) of the correction C[y][x] = c(y) c(x): 1 / t((x - N div 2) / N) inside the trusted region 8 |x - N div 2| <= 3 N,
// 0 outside it; t(f) = exp(beta (sqrt(1 - 4 f^2) - 1)), beta = 1.15 K
__device__ __forceinline__ double idg_taper(double f, int K) { return exp(1.15 * (double)K * (sqrt(1.0 - 4.0 * f * f) - 1.0)); }
__device__ __forceinline__ double idg_correction(int64_t x, int64_t N, int K)
{
    const int64_t d = x - N / 2;
    if (8 * (d < 0 ? -d : d) > 3 * N) return 0.0;
    return 1.0 / idg_taper((double)d / (double)N, K);
}

}  // namespace gridhip
