// The antenna fit of gridhip_fringe_solve (fringe_solve.hip) as a driver enqueues it: the fit drivers of fringe.hip and
// tec.hip run the same solve between their searches (delay_common.h, "the fit driver"; include/gridhip.h, "dispersive
// delay (TEC) calibration": the fit is gridhip_fringe_solve, unchanged).
#pragma once
#include "common.h"

namespace gridhip {

// one end of a used baseline as its antenna sees it: side 0, the antenna is p and `other` is q; side 1 the reverse
struct FrEdge {
    double w, tau, r, zr, zi;
    int other, side;
};

struct FrSolve {
    int B, I, A;
    const int64_t *a1, *a2;
    const double *peaks;
    double min_count, min_coh2;
    int refant, niter;
    double tol;
    double *sol, *info;
    double *w;     // [I][B]: the baseline weights
    double *part;  // [I][8]: what an interval adds to the stats
    FrEdge *edges;  // [I][2 B]: the antennas' lists of their used baselines
    const double *gate;  // the driver: the stats of the search before; [7] set: that search did not run, nor does the solve
};

// the scalar rules of gridhip_fringe_solve
bool fr_solve_args_ok(int64_t B, int64_t I, int64_t A, double min_count, double min_coh2, int64_t refant, int64_t niter,
                      double tol);
// the two launches of a solve on the context's stream; stats: 8 doubles on the device
void fr_solve_launch(gridhip_ctx *ctx, const FrSolve &a, double *stats);
// sol[n][4] = { 0, 0, 1, 0 }
void fr_init_sol_launch(gridhip_ctx *ctx, int64_t n, double *sol);

}  // namespace gridhip
