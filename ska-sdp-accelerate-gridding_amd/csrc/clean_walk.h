// What the four CLEANs (clean.hip, msclean.hip, mfclean.hip, jclean.hip) share and nothing else includes: the tile, a
// tile's table entry, the search rule and its reductions, the stop level of the _auto forms, the one walk over a tile
// that all four tile kernels are, and on the host the tile grids and the launch loop of a call.
#pragma once
#include <type_traits>

#include "imaging.h"

namespace gridhip {

constexpr int CLEAN_TH = 16, CLEAN_TW = 128;  // one wave takes one row of a tile, 16 bytes per lane
static_assert(CLEAN_MAX_N == (int64_t)CLEAN_TH * 65535, "the tile grid's limit");

// The two cells of a slot as one value: storing it is one 16-byte store by construction.  (Two 8-byte stores that the
// compiler is left to pair again are not: with several planes it merges the second of them with the tail cell's store
// in another block, and the pair is lost.)
typedef double clean_pair __attribute__((ext_vector_type(2)));

struct CleanEntry {  // a tile's peak: the signed value and its flat index; k < 0: no cell of the tile can be selected
    double v;
    long long k;
};

__device__ __forceinline__ int64_t lo64(int64_t a, int64_t b) { return a < b ? a : b; }
__device__ __forceinline__ int64_t hi64(int64_t a, int64_t b) { return a > b ? a : b; }

// does (v, k) beat the best so far?  NaN never does; a larger magnitude does, and the lower index among equals
__device__ __forceinline__ void consider(double v, long long k, double &bv, long long &bk)
{
    const double a = fabs(v), b = fabs(bv);
    if (v == v && k >= 0 && (bk < 0 || a > b || (a == b && k < bk))) {
        bv = v;
        bk = k;
    }
}

// the best of a work-group in thread 0 (sh: one entry per wave)
__device__ __forceinline__ void group_best(double &bv, long long &bk, CleanEntry *sh)
{
    for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_down(bv, off);
        const long long ok = __shfl_down(bk, off);
        consider(ov, ok, bv, bk);
    }
    const int wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
    if ((threadIdx.x & 63) == 0) sh[wave] = {bv, bk};
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < nwaves; ++w) consider(sh[w].v, sh[w].k, bv, bk);
}

// the best entry of a tile table in thread 0 of the one work-group that reduces it: the head of every pick kernel
// (comparisons only: nothing here that contraction could change, whichever way the caller is compiled; the running best
// is kept in locals and handed out at the end, which is what keeps the pick kernels at the registers they had)
__device__ __forceinline__ void table_best(const CleanEntry *table, int ntiles, double &bv, long long &bk,
                                           CleanEntry *sh)
{
    double v = 0.0;
    long long k = -1;
    for (int t = threadIdx.x; t < ntiles; t += blockDim.x) consider(table[t].v, table[t].k, v, k);
    group_best(v, k, sh);
    bv = v, bk = k;
}

// The stop level of an _auto call, by the first pick kernel: T = max(threshold, nsigma * sigma, peak_frac * |p1|), each
// product rounded once, a term whose factor is 0 left out (noise is then not read); p1 is NaN when nothing can be
// selected and its term is then left out.  *bad: nsigma > 0 and sigma is NaN - T is NaN and the call stops at once.
__device__ __forceinline__ double stop_level(double threshold, double nsigma, const double *noise, double peak_frac,
                                             double p1, bool *bad)
{
    double T = threshold;
    *bad = false;
    if (nsigma > 0.0) {
        const double sigma = *noise;
        if (sigma != sigma) {
            *bad = true;
            return sigma;
        }
        const double a = nsigma * sigma;
        T = a > T ? a : T;
    }
    if (peak_frac > 0.0 && p1 == p1) {
        const double b = peak_frac * fabs(p1);
        T = b > T ? b : T;
    }
    return T;
}

// One tile per work-group of 256: the body of clean_tile_kernel, ms_tile_kernel, mf_tile_kernel and j_tile_kernel.  SUB = false: grid
// (ntx, nty), the tile's entry from the residual as it is.  SUB = true: the grid covers the most tiles the update
// region can overlap, counted from the region's first tile; work-groups past its last tile leave.  The update region is
// the cells whose PSF index lies in the grid when the PSF's centre is put on the component at flat index k, cut to the
// patch when patch > 0.  Every cell of the tile is read (its entry is over the whole tile), the cells of the region are
// updated and stored.  A lane takes the two cells of one 16-byte slot of the row, in all T residual planes and - inside
// the region - all NP PSF planes; the slots are those of plane 0, aligned by construction, and a row whose first or
// last cell shares its slot with the neighbouring tile (odd N, or a base address that is 8 bytes off) takes that cell
// alone.  For odd N the further planes are 8 bytes apart in alignment: one that is not aligned where plane 0 is takes
// its two cells by two 8-byte accesses.  The PSF is read at a shifted offset: 16 bytes at once where that address
// happens to be aligned (the same for a whole wave), two loads if not.  The tile's best (score, index) goes to
// table[ty * ntx + tx].
// The policy p, by value, says what differs between them:
//     T, NP             residual planes and PSF planes
//     res, psf, cells   plane 0 of each and the stride from one plane to the next
//     product(t, q, p)  the q-th of the T rounded products that plane t of a cell loses, from the cell's PSF values
//                       p[NP]; the walk subtracts them one after the other, q ascending, where the cell is in the region
//                       (a product that is the constant +0.0 for some (t, q) costs nothing: both loops are unrolled and
//                       x - (+0.0) is x for every x - the joint CLEAN's planes, which do not mix, rely on it)
//     score(r)          what the search maximises in magnitude, from r[T]
//     searched(a)       whether the cell at flat index a may be selected (the mask; the subtraction does not ask)
// (contraction is off here whatever the caller's setting; the pragma is lexical, so the policy's methods set their own)
template <bool SUB, class Policy>
__device__ __forceinline__ void clean_tile_walk(int64_t N, int64_t border, int64_t patch, int ntx, long long k,
                                                CleanEntry *table, CleanEntry *sh, const Policy p)
{
#pragma clang fp contract(off)
    constexpr int T = Policy::T, NP = Policy::NP;
    int64_t tx = blockIdx.x, ty = blockIdx.y;
    int64_t ylo = 0, yhi = -1, xlo = 0, xhi = -1, py = 0, px = 0;
    const int64_t c = N / 2;
    if (SUB) {
        py = k / N, px = k % N;
        ylo = py - c, yhi = py - c + N - 1, xlo = px - c, xhi = px - c + N - 1;
        if (patch > 0) {
            ylo = hi64(ylo, py - patch), yhi = lo64(yhi, py + patch);
            xlo = hi64(xlo, px - patch), xhi = lo64(xhi, px + patch);
        }
        ylo = hi64(ylo, 0), yhi = lo64(yhi, N - 1), xlo = hi64(xlo, 0), xhi = lo64(xhi, N - 1);
        ty += ylo / CLEAN_TH, tx += xlo / CLEAN_TW;
        if (ty > yhi / CLEAN_TH || tx > xhi / CLEAN_TW) return;
    }
    double *const res = p.res;
    const double *const psf = p.psf;
    const int64_t cells = p.cells;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t x0 = tx * CLEAN_TW, x1 = lo64(x0 + CLEAN_TW, N);
    const int64_t mis = (int64_t)(((uintptr_t)res >> 3) & 1);  // res + a is 16-byte aligned where a + mis is even
    double bv = 0.0;
    long long bk = -1;
    for (int r = wave; r < CLEAN_TH; r += 4) {
        const int64_t y = ty * CLEAN_TH + r;
        if (y >= N) break;
        const int64_t base = y * N;
        const bool yin = SUB && y >= ylo && y <= yhi, ysearch = y >= border && y < N - border;
        const int64_t poff = (y - py + c) * N + (c - px) - base;  // psf index of the cell at flat index a: a + poff
        const int64_t a0 = ((base + x0 + mis) & ~(int64_t)1) - mis, a1 = base + x1;
        for (int64_t a = a0 + 2 * lane; a < a1; a += 128) {
            const int64_t x = a - base;
            const bool v0 = x >= x0, v1 = x + 1 < x1;  // (at least one holds: a slot has a cell of this tile's row)
            double r0[T], r1[T];
#pragma unroll
            for (int t = 0; t < T; ++t) {
                const double *q = res + t * cells + a;
                r0[t] = 0.0, r1[t] = 0.0;
                if (v0 && v1 && (t == 0 || ((uintptr_t)q & 15) == 0)) {
                    const double2 w = *reinterpret_cast<const double2 *>(q);
                    r0[t] = w.x, r1[t] = w.y;
                } else if (T == 1) {  // (plane 0 alone: exactly one of the two cells)
                    if (v0)
                        r0[t] = q[0];
                    else
                        r1[t] = q[1];
                } else {
                    if (v0) r0[t] = q[0];
                    if (v1) r1[t] = q[1];
                }
            }
            if (yin) {
                const bool u0 = v0 && x >= xlo && x <= xhi, u1 = v1 && x + 1 >= xlo && x + 1 <= xhi;
                if (u0 || u1) {
                    double p0[NP], p1[NP];
#pragma unroll
                    for (int s = 0; s < NP; ++s) {
                        const double *q = psf + s * cells + (a + poff);
                        p0[s] = 0.0, p1[s] = 0.0;
                        if (u0 && u1 && ((uintptr_t)q & 15) == 0) {
                            const double2 w = *reinterpret_cast<const double2 *>(q);
                            p0[s] = w.x, p1[s] = w.y;
                        } else {
                            if (u0) p0[s] = q[0];
                            if (u1) p1[s] = q[1];
                        }
                    }
#pragma unroll
                    for (int t = 0; t < T; ++t) {
#pragma unroll
                        for (int q = 0; q < T; ++q) {  // (each product is rounded, then subtracted)
                            if (u0) r0[t] = r0[t] - p.product(t, q, p0);
                            if (u1) r1[t] = r1[t] - p.product(t, q, p1);
                        }
                        double *o = res + t * cells + a;
                        if (u0 && u1 && (t == 0 || ((uintptr_t)o & 15) == 0)) {
                            *reinterpret_cast<clean_pair *>(o) = clean_pair{r0[t], r1[t]};
                        } else if (T == 1) {
                            if (u0)
                                o[0] = r0[t];
                            else
                                o[1] = r1[t];
                        } else {
                            if (u0) o[0] = r0[t];
                            if (u1) o[1] = r1[t];
                        }
                    }
                }
            }
            if (ysearch) {
                if (v0 && x >= border && x < N - border && p.searched(a)) consider(p.score(r0), a, bv, bk);
                if (v1 && x + 1 >= border && x + 1 < N - border && p.searched(a + 1)) consider(p.score(r1), a + 1, bv, bk);
            }
        }
    }
    group_best(bv, bk, sh);
    if (threadIdx.x == 0) table[ty * ntx + tx] = {bv, bk};
}

// The policy of one residual and one PSF (Hogbom, and each slice of the multi-scale CLEAN): the one product is f * psf,
// rounded before the walk subtracts it; the score is the value itself.  MASK: a cell whose mask byte is 0 is not
// searched (a lane reads the two bytes of its slot, in searched rows only); without MASK no byte is read.
template <bool MASK>
struct OneTermWalk {
    static constexpr int T = 1, NP = 1;
    double *res;
    const double *psf;
    int64_t cells;  // (not used: there is no second plane)
    double f;
    const uint8_t *mask;
    __device__ __forceinline__ double product(int, int, const double (&p)[1]) const
    {
#pragma clang fp contract(off)
        return f * p[0];
    }
    __device__ __forceinline__ double score(const double (&r)[1]) const { return r[0]; }
    __device__ __forceinline__ bool searched(int64_t a) const { return !MASK || mask[a] != 0; }
};

// ---- the host side of a call ----------------------------------------------------------------------------------------
// the most tiles of side T an interval of L cells overlaps, wherever it starts (at most all `have` of them)
static inline int64_t tiles_spanned(int64_t L, int64_t T, int64_t have)
{
    const int64_t t = (L + T - 2) / T + 1;
    return t < have ? t : have;
}

// The tile grids of an N x N clean: all tiles (the first pass), and the most tiles an update region can overlap - the
// whole PSF, or the patch when it is smaller (every later pass).
struct CleanTiles {
    int ntx, nty, ntiles;
    dim3 all, part;
};
static inline CleanTiles clean_tiles(int64_t N, int64_t patch = 0)
{
    const int64_t ntx = (N + CLEAN_TW - 1) / CLEAN_TW, nty = (N + CLEAN_TH - 1) / CLEAN_TH;
    const int64_t span = patch > 0 && 2 * patch + 1 < N ? 2 * patch + 1 : N;
    return {(int)ntx, (int)nty, (int)(ntx * nty), dim3((unsigned)ntx, (unsigned)nty),
            dim3((unsigned)tiles_spanned(span, CLEAN_TW, ntx), (unsigned)tiles_spanned(span, CLEAN_TH, nty))};
}

// The launches of one call, in stream order: the tile pass over all tiles and the first pick, then niter times the tile
// pass over the update region and the next pick - enqueued unconditionally; the state block on the device stops them.
// The four callables launch the caller's kernels (a caller makes each pair from one generic lambda that takes the
// template flag as a std::true_type or std::false_type).
template <class Tile0, class Pick0, class Tile, class Pick>
static inline void clean_launch_loop(int64_t niter, Tile0 first_tile, Pick0 first_pick, Tile tile, Pick pick)
{
    first_tile();
    first_pick();
    for (int64_t i = 0; i < niter; ++i) {
        tile();
        pick();
    }
}

}  // namespace gridhip
