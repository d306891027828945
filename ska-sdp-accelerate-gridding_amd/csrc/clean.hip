// Hogbom CLEAN, the minor cycle between two major cycles (include/gridhip.h, "deconvolution").  Everything stays on the
// device: the stop condition lives in a small state block, the host enqueues niter iterations unconditionally and reads
// nothing back, and a launch whose state is stopped returns at its first instruction.
//
// The image is cut into tiles of CLEAN_TH rows x CLEAN_TW columns and a device table keeps each tile's peak under the
// search rule (largest |value| inside the border, ties to the lowest flat index, NaN never).  One call is
//     clean_tile_kernel<false>   builds the table: one pass over the residual
//     clean_pick_kernel<true>    zeroes the state, reduces the table to the peak, takes the first component
//     niter x { clean_tile_kernel<true>   subtracts the shifted, scaled PSF from the tiles the PSF (or the patch) overlaps
//                                         - the launch covers those tiles only - and recomputes their entries in the same pass
//               clean_pick_kernel<false>  reduces the table to the next peak, tests the stop rule, takes the next component }
// An iteration therefore reads the residual once, the PSF once and writes the residual once over the overlapped region
// (24 B per cell), plus 16 B per tile of table; with patch > 0 that is the patch area plus the table, not N^2.
// The table crosses from the tile kernel to the pick kernel at a kernel boundary: every work-group's entry is visible to
// the one work-group that reduces them without any fence or ticket inside a launch, and no launch ever waits on another
// work-group, so nothing depends on how many work-groups are resident.
// Determinism: every comparison is (|value|, lower flat index wins), in the lanes, across a wave, across a work-group and
// across the table alike, so the peak does not depend on scheduling; there is no atomic in this file.  The subtraction
// rounds f * psf before it subtracts (contraction is off), so that a plain restatement in numpy gives the same bits.
#include "common.h"
#include "imaging.h"

namespace gridhip {

namespace {

// (the tile, CleanEntry, consider and group_best are in imaging.h: msclean.hip shares them)
struct CleanState {  // 64 bytes at the head of the scratch block
    double peak;          // the residual's current peak (signed); NaN when no cell can be selected
    long long k;          // its flat index, -1 when none
    long long iters;      // components taken so far
    double flux;          // sum of the f added to the model
    double f;             // gain * peak of the component the next tile kernel subtracts
    long long stopped;    // threshold reached, out of iterations or nothing to select: every later launch returns
    double T;             // the stop level (the _auto forms: the first pick computes it; else the threshold)
    long long reason;     // why the loop stopped (the _auto forms' codes)
};

// One tile per work-group.  SUB = false: grid (ntx, nty), the tile's entry from the residual as it is.  SUB = true: the
// grid covers the most tiles the update region can overlap, counted from the region's first tile; work-groups past its
// last tile leave.  The update region is the cells whose PSF index lies in the grid, cut to the patch when patch > 0.
// Every cell of the tile is read (its entry is over the whole tile), the cells of the region are updated and stored.
// A lane takes the two cells of one 16-byte aligned slot of the row; a row whose first or last cell shares its slot with
// the neighbouring tile (odd N, or a base address that is 8 bytes off) takes that cell alone.  The PSF is read at a
// shifted offset: 16 bytes at once where that address happens to be aligned (the same for a whole wave), two loads if not.
// MASK: a cell whose mask byte is 0 is not searched (a lane reads the two bytes of its slot, in searched rows only);
// the subtraction does not look at the mask.  Without MASK the kernel is the code it was before there were masks.
template <bool SUB, bool MASK>
__global__ void __launch_bounds__(256)
    clean_tile_kernel(int64_t N, int64_t border, int64_t patch, int ntx, const double *__restrict__ psf, double *res,
                      CleanEntry *__restrict__ table, const CleanState *st, const uint8_t *__restrict__ mask)
{
#pragma clang fp contract(off)
    __shared__ CleanEntry sh[4];
    int64_t tx = blockIdx.x, ty = blockIdx.y;
    int64_t ylo = 0, yhi = -1, xlo = 0, xhi = -1, py = 0, px = 0;
    const int64_t c = N / 2;
    double f = 0.0;
    if (SUB) {
        if (st->stopped) return;
        const int64_t k = st->k;
        f = st->f;
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
            double r0 = 0.0, r1 = 0.0;
            if (v0 && v1) {
                const double2 t = *reinterpret_cast<const double2 *>(res + a);
                r0 = t.x, r1 = t.y;
            } else if (v0) {
                r0 = res[a];
            } else {
                r1 = res[a + 1];
            }
            if (yin) {
                const bool u0 = v0 && x >= xlo && x <= xhi, u1 = v1 && x + 1 >= xlo && x + 1 <= xhi;
                if (u0 || u1) {
                    const double *q = psf + (a + poff);
                    double p0 = 0.0, p1 = 0.0;
                    if (u0 && u1 && ((uintptr_t)q & 15) == 0) {
                        const double2 t = *reinterpret_cast<const double2 *>(q);
                        p0 = t.x, p1 = t.y;
                    } else {
                        if (u0) p0 = q[0];
                        if (u1) p1 = q[1];
                    }
                    if (u0) r0 = r0 - f * p0;
                    if (u1) r1 = r1 - f * p1;
                    if (u0 && u1)
                        *reinterpret_cast<double2 *>(res + a) = make_double2(r0, r1);
                    else if (u0)
                        res[a] = r0;
                    else
                        res[a + 1] = r1;
                }
            }
            if (ysearch) {
                if (v0 && x >= border && x < N - border && (!MASK || mask[a] != 0)) consider(r0, a, bv, bk);
                if (v1 && x + 1 >= border && x + 1 < N - border && (!MASK || mask[a + 1] != 0)) consider(r1, a + 1, bv, bk);
            }
        }
    }
    group_best(bv, bk, sh);
    if (threadIdx.x == 0) table[ty * ntx + tx] = {bv, bk};
}

// One work-group: the table's best is the residual's peak.  Then the head of the next iteration, by thread 0: stop when
// nothing can be selected, when niter components are taken or when |peak| <= threshold - before anything is
// subtracted - else take the component: f = gain * peak into the model, the flux and the state, where the next tile
// kernel finds it.  INIT: the first pick of a call, which starts the state from zero whatever the block held.
// AUTO (the _auto forms): the first pick computes the stop level T from the first peak and the noise and keeps it in the
// state, every pick tests |peak| <= T and records why it stopped - 3: no usable sigma, 2: nothing selectable,
// 1: |peak| <= T, 0: niter components taken, the first that holds - and stats has 8 doubles.
template <bool INIT, bool AUTO>
__global__ void __launch_bounds__(1024)
    clean_pick_kernel(int ntiles, const CleanEntry *__restrict__ table, CleanState *st, double *model, double gain,
                      double threshold, int64_t niter, double *stats, double nsigma, const double *noise, double peak_frac)
{
    __shared__ CleanEntry sh[16];
    if (!INIT && st->stopped) return;
    double bv = 0.0;
    long long bk = -1;
    for (int t = threadIdx.x; t < ntiles; t += blockDim.x) consider(table[t].v, table[t].k, bv, bk);
    group_best(bv, bk, sh);
    if (threadIdx.x != 0) return;
    long long iters = INIT ? 0 : st->iters;
    double flux = INIT ? 0.0 : st->flux;
    const double peak = bk < 0 ? __builtin_nan("") : bv;
    bool bad = false;
    if (AUTO) threshold = INIT ? stop_level(threshold, nsigma, noise, peak_frac, peak, &bad) : st->T;
    const bool stop = bad || bk < 0 || iters >= niter || !(fabs(bv) > threshold);
    if (!stop) {
        // the model cell and the flux receive gain * peak in one fused step each (what contraction made of the two
        // sums from the start, and what the header promises); f, which scales the PSF, is the rounded product
        const double f = gain * bv;
        model[bk] = fma(gain, bv, model[bk]);
        flux = fma(gain, bv, flux);
        iters += 1;
        st->f = f;
    }
    st->peak = peak;
    st->k = bk;
    st->iters = iters;
    st->flux = flux;
    st->stopped = stop ? 1 : 0;
    if (stats) {
        stats[0] = (double)iters;
        stats[1] = peak;
        stats[2] = (double)bk;
        stats[3] = flux;
    }
    if (AUTO) {
        const long long reason = !stop ? 0 : bad ? 3 : bk < 0 ? 2 : !(fabs(bv) > threshold) ? 1 : 0;
        st->T = threshold;
        st->reason = reason;
        if (stats) {
            if (INIT) stats[4] = threshold, stats[6] = peak, stats[7] = 0.0;
            stats[5] = (double)reason;
        }
    }
}

bool overlap(const double *a, const double *b, size_t bytes)
{
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + bytes && y < x + bytes;
}

template <bool MASK, bool AUTO>
void clean_launch(gridhip_ctx *ctx, int64_t N, const double *psf, double *residual, double *model, double gain,
                  double threshold, int64_t niter, int64_t border, int64_t patch, double *stats, void *scratch,
                  const CleanAuto &au)
{
    const int64_t ntx = (N + CLEAN_TW - 1) / CLEAN_TW, nty = (N + CLEAN_TH - 1) / CLEAN_TH;
    CleanState *st = reinterpret_cast<CleanState *>(scratch);
    CleanEntry *table = reinterpret_cast<CleanEntry *>(st + 1);
    const int ntiles = (int)(ntx * nty);
    const int64_t span = patch > 0 && 2 * patch + 1 < N ? 2 * patch + 1 : N;
    const dim3 all((unsigned)ntx, (unsigned)nty);
    const dim3 part((unsigned)tiles_spanned(span, CLEAN_TW, ntx), (unsigned)tiles_spanned(span, CLEAN_TH, nty));
    hipLaunchKernelGGL((clean_tile_kernel<false, MASK>), all, dim3(256), 0, ctx->stream, N, border, patch, (int)ntx, psf,
                       residual, table, (const CleanState *)st, au.mask);
    hipLaunchKernelGGL((clean_pick_kernel<true, AUTO>), dim3(1), dim3(1024), 0, ctx->stream, ntiles,
                       (const CleanEntry *)table, st, model, gain, threshold, niter, stats, au.nsigma, au.noise, au.peak_frac);
    for (int64_t i = 0; i < niter; ++i) {
        hipLaunchKernelGGL((clean_tile_kernel<true, MASK>), part, dim3(256), 0, ctx->stream, N, border, patch, (int)ntx, psf,
                           residual, table, (const CleanState *)st, au.mask);
        hipLaunchKernelGGL((clean_pick_kernel<false, AUTO>), dim3(1), dim3(1024), 0, ctx->stream, ntiles,
                           (const CleanEntry *)table, st, model, gain, threshold, niter, stats, au.nsigma, au.noise,
                           au.peak_frac);
    }
}

}  // namespace

int clean_check(gridhip_ctx *ctx, int64_t N, const double *psf, const double *residual, const double *model, double gain,
                double threshold, int64_t niter, int64_t border, int64_t patch)
{
    if (N < 1 || !(gain > 0.0 && gain <= 1.0) || !(threshold >= 0.0) || niter < 0 || border < 0 || 2 * border >= N ||
        patch < 0 || !psf || !residual || !model)
        return fail(ctx, GRIDHIP_EINVAL, "clean: bad argument");
    if (N > CLEAN_MAX_N) return fail(ctx, GRIDHIP_EUNSUPPORTED, "clean: N above %d", CLEAN_TH * 65535);
    const size_t bytes = (size_t)N * N * 8;
    if (overlap(psf, residual, bytes) || overlap(psf, model, bytes) || overlap(residual, model, bytes))
        return fail(ctx, GRIDHIP_EINVAL, "clean: psf, residual and model must not overlap");
    return GRIDHIP_OK;
}

size_t clean_scratch_bytes(int64_t N)
{
    const int64_t ntx = (N + CLEAN_TW - 1) / CLEAN_TW, nty = (N + CLEAN_TH - 1) / CLEAN_TH;
    return sizeof(CleanState) + (size_t)ntx * nty * sizeof(CleanEntry);
}

int clean_auto_check(gridhip_ctx *ctx, int64_t N, const double *residual, const double *model, const uint8_t *mask,
                     double nsigma, const double *noise, double peak_frac)
{
    if (!(nsigma >= 0.0 && nsigma < __builtin_inf()) || !(peak_frac >= 0.0 && peak_frac < 1.0) || (nsigma > 0.0 && !noise))
        return fail(ctx, GRIDHIP_EINVAL, "clean_auto: bad nsigma, noise or peak_frac");
    if (mask) {
        const uintptr_t m = (uintptr_t)mask, cells = (uintptr_t)N * N;
        for (const double *a : {residual, model})
            if (m < (uintptr_t)a + cells * 8 && (uintptr_t)a < m + cells)
                return fail(ctx, GRIDHIP_EINVAL, "clean_auto: the mask must not overlap residual or model");
    }
    return GRIDHIP_OK;
}

int clean_run(gridhip_ctx *ctx, int64_t N, const double *psf, double *residual, double *model, double gain,
              double threshold, int64_t niter, int64_t border, int64_t patch, double *stats, void *scratch,
              const CleanAuto &au)
{
    if (!au.on)
        clean_launch<false, false>(ctx, N, psf, residual, model, gain, threshold, niter, border, patch, stats, scratch, au);
    else if (au.mask)
        clean_launch<true, true>(ctx, N, psf, residual, model, gain, threshold, niter, border, patch, stats, scratch, au);
    else
        clean_launch<false, true>(ctx, N, psf, residual, model, gain, threshold, niter, border, patch, stats, scratch, au);
    GH_CHECK_HIP(ctx, hipGetLastError());
    return GRIDHIP_OK;
}

}  // namespace gridhip

using namespace gridhip;

namespace {

int clean_any(gridhip_ctx *ctx, bool dev, int64_t N, const double *psf, double *residual, double *model, double gain,
              double threshold, int64_t niter, int64_t border, int64_t patch, double *stats, CleanAuto au = CleanAuto{})
{
    if (!ctx) return GRIDHIP_EINVAL;
    GH_CHECK(clean_check(ctx, N, psf, residual, model, gain, threshold, niter, border, patch));
    if (au.on) GH_CHECK(clean_auto_check(ctx, N, residual, model, au.mask, au.nsigma, au.noise, au.peak_frac));
    GH_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    DevBuf scratch;
    GH_CHECK(scratch.alloc(ctx, clean_scratch_bytes(N)));
    if (dev)
        return clean_run(ctx, N, psf, residual, model, gain, threshold, niter, border, patch, stats, scratch.p, au);
    const size_t bytes = (size_t)N * N * 8, sbytes = au.on ? 64 : 32;
    DevBuf p, r, m, s, mk, nz;
    GH_CHECK(p.upload(ctx, psf, bytes));
    GH_CHECK(r.upload(ctx, residual, bytes));
    GH_CHECK(m.upload(ctx, model, bytes));
    GH_CHECK(s.alloc(ctx, sbytes));
    if (au.mask) {
        GH_CHECK(mk.upload(ctx, au.mask, bytes / 8));
        au.mask = mk.as<uint8_t>();
    }
    if (au.nsigma > 0.0) {
        GH_CHECK(nz.upload(ctx, au.noise, 8));
        au.noise = nz.as<double>();
    }
    GH_CHECK(clean_run(ctx, N, p.as<double>(), r.as<double>(), m.as<double>(), gain, threshold, niter, border, patch,
                       s.as<double>(), scratch.p, au));
    GH_CHECK(d2h(ctx, residual, r.p, bytes));
    GH_CHECK(d2h(ctx, model, m.p, bytes));
    if (stats) GH_CHECK(d2h(ctx, stats, s.p, sbytes));
    return sync(ctx);
}

}  // namespace

extern "C" {

int gridhip_clean(gridhip_ctx *ctx, int64_t N, const double *psf, double *residual, double *model, double gain,
                  double threshold, int64_t niter, int64_t border, int64_t patch, double *stats)
{
    return clean_any(ctx, false, N, psf, residual, model, gain, threshold, niter, border, patch, stats);
}

int gridhip_clean_dev(gridhip_ctx *ctx, int64_t N, const double *psf, double *residual, double *model, double gain,
                      double threshold, int64_t niter, int64_t border, int64_t patch, double *stats)
{
    return clean_any(ctx, true, N, psf, residual, model, gain, threshold, niter, border, patch, stats);
}

int gridhip_clean_auto(gridhip_ctx *ctx, int64_t N, const double *psf, double *residual, double *model, double gain,
                       double threshold, int64_t niter, int64_t border, int64_t patch, const uint8_t *mask, double nsigma,
                       const double *noise, double peak_frac, double *stats)
{
    return clean_any(ctx, false, N, psf, residual, model, gain, threshold, niter, border, patch, stats,
                     CleanAuto{mask, nsigma, noise, peak_frac, true});
}

int gridhip_clean_auto_dev(gridhip_ctx *ctx, int64_t N, const double *psf, double *residual, double *model, double gain,
                           double threshold, int64_t niter, int64_t border, int64_t patch, const uint8_t *mask,
                           double nsigma, const double *noise, double peak_frac, double *stats)
{
    return clean_any(ctx, true, N, psf, residual, model, gain, threshold, niter, border, patch, stats,
                     CleanAuto{mask, nsigma, noise, peak_frac, true});
}

}  // extern "C"
