// The rounded arithmetic, the layout constants and the cube rules of the delay-like calibrations: what the antenna fit
// (fringe_solve.hip) needs of delay_common.h, which includes this file and adds what the searches, the apply steps and
// the fit drivers share.
//
// CONTRACTION IS OFF FROM HERE ON.  The Makefile passes no -ffp-contract flag, so a header's products would fuse by
// default, and every output of these modules is pinned bit for bit to products and sums that are rounded one by one.
// The pragma below, at file scope ahead of the first function, therefore belongs to this header: it holds for the rest of
// the translation unit that includes it.
#pragma once
#include "common.h"

#pragma clang fp contract(off)

namespace gridhip {

namespace {

typedef unsigned long long u64;

constexpr int DL_HEAD = 16, DL_ROW = 12, DL_STATS = 8;  // doubles of a table's head, of a row of peaks, of the stats
constexpr int DL_MAX_A = GRIDHIP_FRINGE_MAX_ANTENNAS;
static_assert(GRIDHIP_FRINGE_HEAD == DL_HEAD && GRIDHIP_TEC_HEAD == DL_HEAD && GRIDHIP_FRINGE_PEAK == DL_ROW &&
                  GRIDHIP_TEC_PEAK == DL_ROW && GRIDHIP_FRINGE_STATS == DL_STATS && GRIDHIP_TEC_STATS == DL_STATS,
              "one layout of the head, the rows and the stats");

__device__ __forceinline__ bool dl_finite(double x) { return __builtin_isfinite(x); }

__device__ __forceinline__ bool dl_int_in(double v, int lo, int hi) { return v >= (double)lo && v <= (double)hi && v == (double)(int)v; }

// exp(2 pi i a b) = (cs, sn): the turns x = a * b reduced to x - rint(x) (exact), then sincospi of twice that
__device__ __forceinline__ double2 dl_phasor(double a, double b)
{
    const double x = a * b;
    const double r = x - rint(x);
    double sn, cs;
    sincospi(2.0 * r, &sn, &cs);
    return make_double2(cs, sn);
}

// x conj(c): four rounded products, two rounded sums
__device__ __forceinline__ double2 dl_mulc(double2 x, double2 c) { return make_double2(x.x * c.x + x.y * c.y, x.y * c.x - x.x * c.y); }
// x c
__device__ __forceinline__ double2 dl_mul(double2 x, double2 c) { return make_double2(x.x * c.x - x.y * c.y, x.x * c.y + x.y * c.x); }
// acc + e x as rmsynth adds it
__device__ __forceinline__ void dl_mac(double2 &acc, double2 e, double2 x)
{
    acc.x = acc.x + (e.x * x.x - e.y * x.y);
    acc.y = acc.y + (e.x * x.y + e.y * x.x);
}

// the second half of the parabola rule of gridhip_rmclean: the offset in cells from the three powers, 0 where it does not apply
__device__ __forceinline__ double dl_parabola(double pm, double ps, double pp)
{
    const double d = (pm - ps) + (pp - ps);
    return d < 0.0 ? (0.5 * (pm - pp)) / d : 0.0;
}

// is (q, qj, qk) ahead of (p, pj, pk)?  The largest power, then the lowest cell of the first axis, then of the second; a
// "none" (-1, -1, -1) is behind everything, and a NaN is ahead of nothing
__device__ __forceinline__ bool dl_ahead(double q, int qj, int qk, double p, int pj, int pk)
{
    return q > p || (q == p && (qj < pj || (qj == pj && qk < pk)));
}

inline bool dl_cube_ok(int64_t B, int64_t T, int64_t F, int64_t A, int64_t max_f) { return B >= 1 && T >= 1 && F >= 1 && F <= max_f && A >= 2; }

// EUNSUPPORTED beyond these: the kernels index baselines and time steps with 32 bits
inline bool dl_cube_fits(int64_t B, int64_t T, int64_t A) { return B <= (1 << 24) && T <= (1 << 20) && A <= DL_MAX_A; }

}  // namespace

}  // namespace gridhip
