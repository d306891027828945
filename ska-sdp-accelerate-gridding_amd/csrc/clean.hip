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
// The tile, the table entry, the search rule and the walk over a tile that the tile kernel is are in clean_walk.h, shared
// with msclean.hip and mfclean.hip; this file has the state, the stop rule and the entry points.
#include "common.h"
#include "clean_walk.h"

namespace gridhip {

namespace {

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

// One tile per work-group: clean_tile_walk (clean_walk.h) on the one residual and the one PSF.  SUB = false: the tile's
// entry from the residual as it is.  SUB = true: f * psf, shifted to the component the state names, is subtracted over
// the update region first.  MASK: a cell whose mask byte is 0 is not searched; the subtraction does not look at the mask.
// Without MASK the kernel is the code it was before there were masks.
template <bool SUB, bool MASK>
__global__ void __launch_bounds__(256)
    clean_tile_kernel(int64_t N, int64_t border, int64_t patch, int ntx, const double *__restrict__ psf, double *res,
                      CleanEntry *__restrict__ table, const CleanState *st, const uint8_t *__restrict__ mask)
{
    __shared__ CleanEntry sh[4];
    if (SUB && st->stopped) return;
    clean_tile_walk<SUB>(N, border, patch, ntx, SUB ? st->k : 0, table, sh,
                         OneTermWalk<MASK>{res, psf, 0, SUB ? st->f : 0.0, mask});
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
    double bv;
    long long bk;
    table_best(table, ntiles, bv, bk, sh);
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

template <bool MASK, bool AUTO>
void clean_launch(gridhip_ctx *ctx, int64_t N, const double *psf, double *residual, double *model, double gain,
                  double threshold, int64_t niter, int64_t border, int64_t patch, double *stats, void *scratch,
                  const CleanAuto &au)
{
    const CleanTiles t = clean_tiles(N, patch);
    CleanState *st = reinterpret_cast<CleanState *>(scratch);
    CleanEntry *table = reinterpret_cast<CleanEntry *>(st + 1);
    const auto tile = [&](auto sub, const dim3 &grid) {
        hipLaunchKernelGGL((clean_tile_kernel<decltype(sub)::value, MASK>), grid, dim3(256), 0, ctx->stream, N, border,
                           patch, t.ntx, psf, residual, table, (const CleanState *)st, au.mask);
    };
    const auto pick = [&](auto init) {
        hipLaunchKernelGGL((clean_pick_kernel<decltype(init)::value, AUTO>), dim3(1), dim3(1024), 0, ctx->stream,
                           t.ntiles, (const CleanEntry *)table, st, model, gain, threshold, niter, stats, au.nsigma,
                           au.noise, au.peak_frac);
    };
    clean_launch_loop(
        niter, [&] { tile(std::false_type{}, t.all); }, [&] { pick(std::true_type{}); },
        [&] { tile(std::true_type{}, t.part); }, [&] { pick(std::false_type{}); });
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
    if (overlap(psf, bytes, residual, bytes) || overlap(psf, bytes, model, bytes) || overlap(residual, bytes, model, bytes))
        return fail(ctx, GRIDHIP_EINVAL, "clean: psf, residual and model must not overlap");
    return GRIDHIP_OK;
}

size_t clean_scratch_bytes(int64_t N)
{
    return sizeof(CleanState) + (size_t)clean_tiles(N).ntiles * sizeof(CleanEntry);
}

int clean_auto_check(gridhip_ctx *ctx, int64_t N, const double *residual, const double *model, const uint8_t *mask,
                     double nsigma, const double *noise, double peak_frac)
{
    if (!(nsigma >= 0.0 && nsigma < __builtin_inf()) || !(peak_frac >= 0.0 && peak_frac < 1.0) || (nsigma > 0.0 && !noise))
        return fail(ctx, GRIDHIP_EINVAL, "clean_auto: bad nsigma, noise or peak_frac");
    if (mask) {
        const size_t cells = (size_t)N * N;
        for (const double *a : {residual, model})
            if (overlap(mask, cells, a, cells * 8))
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
    const size_t bytes = (size_t)N * N * 8;
    Staged st(ctx, dev);
    psf = st.in(psf, bytes), residual = st.inout(residual, residual, bytes), model = st.inout(model, model, bytes);
    stats = st.out(stats, au.on ? 64 : 32), au.mask = st.in(au.mask, bytes / 8);
    if (au.nsigma > 0.0) au.noise = st.in(au.noise, 8);
    GH_CHECK(st.status());
    GH_CHECK(clean_run(ctx, N, psf, residual, model, gain, threshold, niter, border, patch, stats, scratch.p, au));
    return st.finish();
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
