// Full-polarisation calibration (include/gridhip.h, "polarisation"): 2x2 Jones matrices per (solution interval, antenna)
// by the matrix StEFCal, their application to a four-correlation stream, and the change between correlations and Stokes
// parameters.  The scheme of a solve is gaincal.hip's - the stop condition lives in the state block, niter iterations are
// enqueued unconditionally and a launch that finds the state stopped returns at its first instruction; nothing is read back.
//
//     jones_init_kernel      the [T][A][12] table and the solved flags start from zero, the gains from I; a warm start in
//                            the diagonal modes has its off-diagonals replaced by +0.0 (a kernel: no memset node)
//     jones_prepare_kernel   one pass over V, M, s, a1, a2, slot: the packed 8-byte key and the weight (0 where the sample
//                            is not used) per visibility, 16 B, and the sums that do not depend on the gains (chi^2 at
//                            G = I, used, flagged, dropped) - one row of partial sums per work-group, no atomics
//     gaincal_begin_kernel   (gain_common.h) adds the rows in a fixed order and starts the state block
//     niter x { jones_iter_kernel    streams key, s, V, M (144 B per visibility: V and M are the caller's arrays - a product
//                                    of them cannot be formed once per solve as gaincal's X and Y are, the gain stands
//                                    between them).  A work-group takes a contiguous range of whole chunks of GC_CHUNK
//                                    visibilities, keeps the gains (8 doubles) and the sums (12 doubles) of ONE interval's
//                                    antennas in dynamic LDS, 160 A bytes, adds with LDS fp64 atomics (24 per visibility)
//                                    and flushes to the global table when the interval changes and at the end of its
//                                    range.  The interval logic is gc_walk (gain_common.h).  A CU holds 1024 threads of it
//                                    whatever the table takes: four work-groups of 256 threads while four tables (and
//                                    a word each) fit, A <= 255, two of 512 up to A = 511, one of 1024 at A = JC_LDS_A
//                                    = 512, exactly 80 KB.
//                                    A > JC_LDS_A: jones_iter_global_kernel adds to the global table directly.
//               jones_update_kernel  one work-group: G' from the table (the LDL^H of the 2x2 den, or its diagonal), the
//                                    phase-only and averaging rules, rel in a fixed order, the stop test; zeroes the table }
//     gc_finish_kernel       (gain_common.h) one work-group: the common phase of the reference antenna, the unsolved (t, a)
//     jones_chi_kernel       one pass with the final gains: chi^2 as partial rows
//     gaincal_stats_kernel   (gain_common.h) the 8 doubles
//     jones_apply_kernel     gridhip_apply_jones;  stokes_kernel  gridhip_stokes - one visibility per lane, no scratch
// Determinism: the table's sums meet in fp64 atomics (LDS, then global), so gains agree to the order of those sums and not
// bit for bit; rel, chi^2 and the counts are added in a fixed order given the gains.  Contraction is off everywhere: every
// product and every sum the header names is rounded on its own.
#include "gain_common.h"

namespace gridhip {

namespace {

constexpr int JC_SUMS = 12;           // num (4 complex), d00, d11, d01 (complex)

struct J2 {  // a 2x2 complex matrix, row-major: 00, 01, 10, 11
    double2 e[4];
};

__device__ __forceinline__ double2 cadd(double2 a, double2 b) { return make_double2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ double2 csub(double2 a, double2 b) { return make_double2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ double2 cconj(double2 a) { return make_double2(a.x, -a.y); }

// C = X Y: C[i][j] = X[i][0] Y[0][j] + X[i][1] Y[1][j], each complex product rounded (cmul), then the two added
__device__ __forceinline__ J2 jmul(const J2 &x, const J2 &y)
{
    J2 c;
    c.e[0] = cadd(cmul(x.e[0], y.e[0]), cmul(x.e[1], y.e[2]));
    c.e[1] = cadd(cmul(x.e[0], y.e[1]), cmul(x.e[1], y.e[3]));
    c.e[2] = cadd(cmul(x.e[2], y.e[0]), cmul(x.e[3], y.e[2]));
    c.e[3] = cadd(cmul(x.e[2], y.e[1]), cmul(x.e[3], y.e[3]));
    return c;
}
__device__ __forceinline__ J2 jherm(const J2 &x)  // X^H (exact)
{
    J2 c;
    c.e[0] = cconj(x.e[0]), c.e[1] = cconj(x.e[2]), c.e[2] = cconj(x.e[1]), c.e[3] = cconj(x.e[3]);
    return c;
}
__device__ __forceinline__ J2 jload(const double2 *p)
{
    J2 c;
    c.e[0] = p[0], c.e[1] = p[1], c.e[2] = p[2], c.e[3] = p[3];
    return c;
}
__device__ __forceinline__ void jstore(double2 *p, const J2 &c) { p[0] = c.e[0], p[1] = c.e[1], p[2] = c.e[2], p[3] = c.e[3]; }
// |X|_F^2, the four |.|^2 added in the order 00, 01, 10, 11
__device__ __forceinline__ double jnorm2(const J2 &x)
{
#pragma clang fp contract(off)
    return ((norm2(x.e[0]) + norm2(x.e[1])) + norm2(x.e[2])) + norm2(x.e[3]);
}
__device__ __forceinline__ J2 jsub(const J2 &x, const J2 &y)
{
    J2 c;
    for (int i = 0; i < 4; ++i) c.e[i] = csub(x.e[i], y.e[i]);
    return c;
}

// cells: T * A.  The table (12 doubles per cell) and the flags are zeroed.  Cold: G = I.  Warm: the gains stay, but for the
// off-diagonals in the diagonal modes, which become +0.0.
__global__ void __launch_bounds__(256)
    jones_init_kernel(int64_t cells, int warm, int mode, double *__restrict__ table, unsigned int *__restrict__ ever,
                      double2 *__restrict__ g)
{
    const int64_t k0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, step = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = k0; e < cells * JC_SUMS; e += step) table[e] = 0.0;
    for (int64_t e = k0; e < cells; e += step) {
        ever[e] = 0u;
        if (!warm) g[4 * e] = make_double2(1.0, 0.0), g[4 * e + 3] = make_double2(1.0, 0.0);
        if (!warm || mode != 0) g[4 * e + 1] = make_double2(0.0, 0.0), g[4 * e + 2] = make_double2(0.0, 0.0);
    }
}

__global__ void __launch_bounds__(256)
    jones_prepare_kernel(int64_t n, int64_t A, int64_t T, const int64_t *__restrict__ a1, const int64_t *__restrict__ a2,
                         const int64_t *__restrict__ slot, const double2 *__restrict__ vis,
                         const double2 *__restrict__ mod, const double *__restrict__ wt, double *__restrict__ S,
                         unsigned long long *__restrict__ key, double *__restrict__ parts)
{
#pragma clang fp contract(off)
    __shared__ double lds[16];
    const int64_t k0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, step = (int64_t)gridDim.x * blockDim.x;
    double chi0 = 0.0;
    unsigned int used = 0, flagged = 0, dropped = 0;  // (a lane sees far fewer than 2^32 visibilities)
    for (int64_t k = k0; k < n; k += step) {
        int64_t p, q, t;
        double s;
        const int c = classify(k, A, T, a1, a2, slot, wt, &p, &q, &t, &s);
        used += c == 0, flagged += c == 1, dropped += c == 2;
        unsigned long long kk = 0ull;
        if (c == 0) {
            chi0 += s * jnorm2(jsub(jload(vis + 4 * k), jload(mod + 4 * k)));
            kk = gc_pack(p, q, t);
        }
        S[k] = c == 0 ? s : 0.0, key[k] = kk;
    }
    gc_prepare_tail(chi0, used, flagged, dropped, parts, lds);
}

// One side of one visibility into the 12 sums of its antenna: Z = Mx Gh, sZ = s Z, num += Y (sZ)^H, den += Z (sZ)^H, of
// which the real parts of 00 and 11 and the entry 01 are kept.  Toward p: Y = V, Mx = M, Gh = G_q^H; toward q: Y = V^H,
// Mx = M^H, Gh = G_p^H.
__device__ __forceinline__ void jones_add(double *row, const J2 &Y, const J2 &Mx, const J2 &Gh, double s)
{
#pragma clang fp contract(off)
    const J2 Z = jmul(Mx, Gh);
    J2 sZ;
    for (int i = 0; i < 4; ++i) sZ.e[i] = make_double2(s * Z.e[i].x, s * Z.e[i].y);
    const J2 sZh = jherm(sZ);
    const J2 N = jmul(Y, sZh);
    for (int i = 0; i < 4; ++i) atomicAdd(&row[2 * i], N.e[i].x), atomicAdd(&row[2 * i + 1], N.e[i].y);
    const double d00 = cmul(Z.e[0], sZh.e[0]).x + cmul(Z.e[1], sZh.e[2]).x;
    const double d11 = cmul(Z.e[2], sZh.e[1]).x + cmul(Z.e[3], sZh.e[3]).x;
    const double2 d01 = cadd(cmul(Z.e[0], sZh.e[1]), cmul(Z.e[1], sZh.e[3]));
    atomicAdd(&row[8], d00), atomicAdd(&row[9], d11), atomicAdd(&row[10], d01.x), atomicAdd(&row[11], d01.y);
}

// both sides of visibility k, one after the other: gp, gq point at the gains of its two antennas, rp, rq at their sums
__device__ __forceinline__ void jones_visibility(int64_t k, double s, const double2 *__restrict__ vis,
                                                 const double2 *__restrict__ mod, const double2 *gp, const double2 *gq,
                                                 double *rp, double *rq)
{
    const J2 V = jload(vis + 4 * k), M = jload(mod + 4 * k);
    jones_add(rp, V, M, jherm(jload(gq)), s);
    jones_add(rq, jherm(V), jherm(M), jherm(jload(gp)), s);
}

// What gc_walk needs of this module: lg [A][4] complex, acc [A][12].  One visibility at a time: unrolled, the 16 doubles of
// V and M of all four would be held at once.  JcSolve below adds the driver's part.
struct JcMod {
    static constexpr int NS = JC_SUMS, NG = 4, GSTEP = 4, UNROLL = 1;
    struct In {
        const double *S;
        const double2 *vis, *mod;
    };
    using Held = GcNoHeld;
    static __device__ __forceinline__ void load_gains(double2 *lg, const double2 *__restrict__ g, long long tn, int A, int64_t)
    {
        gc_copy_gains(lg, g, tn, 4 * A);
    }
    static __device__ __forceinline__ void add(const In &in, const Held &, int, int64_t k, const double2 *gp,
                                               const double2 *gq, int64_t, double *rp, double *rq)
    {
        jones_visibility(k, in.S[k], in.vis, in.mod, gp, gq, rp, rq);
    }
};

// One iteration's sums, A <= JC_LDS_A: gc_walk with dynamic LDS, 160 bytes per antenna
__global__ void __launch_bounds__(1024)
    jones_iter_kernel(int64_t n, int A, int64_t per, const double *__restrict__ S, const unsigned long long *__restrict__ key,
                      const double2 *__restrict__ vis, const double2 *__restrict__ mod, const double2 *__restrict__ g,
                      double *table, const GcState *st)
{
    extern __shared__ double2 jc_lds[];
    gc_walk<JcMod>(JcMod::In{S, vis, mod}, n, A, 1, per, key, g, table, st, jc_lds,
                   reinterpret_cast<double *>(jc_lds + (size_t)4 * A));
}

__global__ void __launch_bounds__(256)
    jones_iter_global_kernel(int64_t n, int64_t A, const double *__restrict__ S, const unsigned long long *__restrict__ key,
                             const double2 *__restrict__ vis, const double2 *__restrict__ mod,
                             const double2 *__restrict__ g, double *table, const GcState *st)
{
    gc_walk_global<JcMod>(JcMod::In{S, vis, mod}, n, A, 1, key, g, table, st);
}

// One work-group of 1024 threads: thread i takes the cells i, i + 1024, ... in order.  An unsolved cell keeps the bits of
// its gain.  den = [[d00, d01], [conj d01, d11]] = L diag(d00, e) L^H with c = d01 / d00 = conj(L[1][0]) and
// e = d11 - |d01|^2 / d00;  G' den = num row by row: x1 = (n1 - n0 c) / e, x0 = n0 / d00 - x1 conj(c).
__global__ void __launch_bounds__(1024)
    jones_update_kernel(int64_t cells, int mode, double tol, double *__restrict__ table, unsigned int *__restrict__ ever,
                        double2 *__restrict__ g, GcState *st)
{
#pragma clang fp contract(off)
    if (st->stopped) return;
    __shared__ double lds[16];
    const bool odd = (st->iters & 1) != 0;
    double d2 = 0.0, s2 = 0.0;
    for (int64_t c = threadIdx.x; c < cells; c += 1024) {
        double *row = table + c * JC_SUMS;
        J2 N;
        for (int i = 0; i < 4; ++i) N.e[i] = make_double2(row[2 * i], row[2 * i + 1]);
        const double d00 = row[8], d11 = row[9];
        const double2 d01 = make_double2(row[10], row[11]);
        for (int i = 0; i < JC_SUMS; ++i) row[i] = 0.0;
        const J2 go = jload(g + 4 * c);
        J2 gn = go;
        bool ok = d00 > 0.0 && d11 > 0.0;
        if (mode == 0) {
            const double e = d11 - norm2(d01) / d00;
            ok = ok && e > 1e-12 * d11;
            if (ok) {
                const double2 cc = make_double2(d01.x / d00, d01.y / d00);
                for (int i = 0; i < 2; ++i) {
                    const double2 n0 = N.e[2 * i], n1 = N.e[2 * i + 1];
                    const double2 w = csub(n1, cmul(n0, cc));
                    const double2 x1 = make_double2(w.x / e, w.y / e);
                    gn.e[2 * i] = csub(make_double2(n0.x / d00, n0.y / d00), cmulc(x1, cc));
                    gn.e[2 * i + 1] = x1;
                }
            }
        } else if (ok) {
            gn.e[0] = make_double2(N.e[0].x / d00, N.e[0].y / d00);
            gn.e[3] = make_double2(N.e[3].x / d11, N.e[3].y / d11);
            gn.e[1] = gn.e[2] = make_double2(0.0, 0.0);
            if (mode == 2)
                for (int i = 0; i < 4; i += 3) {
                    const double a = sqrt(norm2(gn.e[i]));
                    gn.e[i] = a > 0.0 ? make_double2(gn.e[i].x / a, gn.e[i].y / a) : go.e[i];
                }
        }
        if (ok) {
            ever[c] = 1u;
            if (odd)
                for (int i = 0; i < 4; ++i)
                    gn.e[i] = make_double2((gn.e[i].x + go.e[i].x) / 2.0, (gn.e[i].y + go.e[i].y) / 2.0);
            jstore(g + 4 * c, gn);
        }
        d2 += jnorm2(jsub(gn, go));
        s2 += jnorm2(gn);
    }
    gc_close_iteration(d2, s2, tol, st, lds);
}

// chi^2 over the used visibilities with the final gains, one partial sum per work-group: s |V - (G_p M) G_q^H|_F^2
__global__ void __launch_bounds__(256)
    jones_chi_kernel(int64_t n, int64_t A, const double *__restrict__ S, const unsigned long long *__restrict__ key,
                     const double2 *__restrict__ g, const double2 *__restrict__ vis, const double2 *__restrict__ mod,
                     double *__restrict__ parts)
{
#pragma clang fp contract(off)
    __shared__ double lds[16];
    const int64_t k0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, step = (int64_t)gridDim.x * blockDim.x;
    double chi = 0.0;
    for (int64_t k = k0; k < n; k += step) {
        const unsigned long long kk = key[k];
        if (!(kk & GC_USED)) continue;
        const int64_t t = (int64_t)(kk >> 42 & GC_FIELD), p = t * A + (int64_t)(kk & GC_FIELD),
                      q = t * A + (int64_t)(kk >> 21 & GC_FIELD);
        const J2 m = jmul(jmul(jload(g + 4 * p), jload(mod + 4 * k)), jherm(jload(g + 4 * q)));
        chi += S[k] * jnorm2(jsub(jload(vis + 4 * k), m));
    }
    chi = block_sum(chi, lds);
    if (threadIdx.x == 0) parts[blockIdx.x] = chi;
}

// det G = g00 g11 - g01 g10 and G^-1 = adj(G) / det G, each entry a conj(det) / |det|^2; nd = |det|^2
__device__ __forceinline__ J2 jinverse(const J2 &x, double *nd)
{
#pragma clang fp contract(off)
    const double2 det = csub(cmul(x.e[0], x.e[3]), cmul(x.e[1], x.e[2]));
    const double dd = norm2(det);
    *nd = dd;
    const double2 adj[4] = {x.e[3], make_double2(-x.e[1].x, -x.e[1].y), make_double2(-x.e[2].x, -x.e[2].y), x.e[0]};
    J2 c;
    for (int i = 0; i < 4; ++i) {
        const double2 h = cmulc(adj[i], det);
        c.e[i] = make_double2(h.x / dd, h.y / dd);
    }
    return c;
}

// gridhip_apply_jones: vout and wout may be vis and wt themselves (element k is read before it is written, by the same
// lane): no __restrict__ on those
__global__ void __launch_bounds__(256)
    jones_apply_kernel(int64_t n, int64_t A, int64_t T, const int64_t *__restrict__ a1, const int64_t *__restrict__ a2,
                       const int64_t *__restrict__ slot, const double2 *__restrict__ g, int inverse, const double2 *vis,
                       const double *wt, double2 *vout, double *wout)
{
#pragma clang fp contract(off)
    const int64_t k0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, step = (int64_t)gridDim.x * blockDim.x;
    for (int64_t k = k0; k < n; k += step) {
        const double s = wt ? wt[k] : 1.0;
        const int64_t p = a1[k], q = a2[k], t = slot ? slot[k] : 0;
        const J2 v = jload(vis + 4 * k);
        J2 o = v;
        double w = inverse ? 0.0 : s;
        if (p >= 0 && p < A && q >= 0 && q < A && t >= 0 && t < T) {
            const J2 gp = jload(g + 4 * (t * A + p)), gq = jload(g + 4 * (t * A + q));
            if (!inverse) {
                o = jmul(jmul(gp, v), jherm(gq));
            } else {
                double np, nq;
                const J2 ip = jinverse(gp, &np), iq = jinverse(gq, &nq);
                if (np > 0.0 && nq > 0.0 && np - np == 0.0 && nq - nq == 0.0) {
                    o = jmul(jmul(ip, v), jherm(iq));
                    w = (s * sqrt(np)) * sqrt(nq);
                }
            }
        }
        jstore(vout + 4 * k, o);
        if (wout) wout[k] = w;
    }
}

// gridhip_stokes: row r of the Stokes block is at rows[r] (null: not selected).  a, b, c, d: the correlations 00, 01, 10,
// 11.  The pair (x, y) of the diagonal is (I, Q) in the linear basis and (I, V) in the circular one; the pair of the
// off-diagonals is (U, V) and (Q, U).
struct StokesRows {
    double2 *r[4];
};
__global__ void __launch_bounds__(256) stokes_kernel(int64_t n, int basis, int inverse, double2 *vis, StokesRows rows)
{
#pragma clang fp contract(off)
    const int dsum = 0, ddif = basis == 0 ? 1 : 3, osum = basis == 0 ? 2 : 1, odif = basis == 0 ? 3 : 2;
    const int64_t k0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, step = (int64_t)gridDim.x * blockDim.x;
    for (int64_t k = k0; k < n; k += step) {
        if (!inverse) {
            const J2 v = jload(vis + 4 * k);
            const double2 a = v.e[0], b = v.e[1], c = v.e[2], d = v.e[3];
            if (rows.r[dsum]) rows.r[dsum][k] = make_double2((a.x + d.x) / 2.0, (a.y + d.y) / 2.0);
            if (rows.r[ddif]) rows.r[ddif][k] = make_double2((a.x - d.x) / 2.0, (a.y - d.y) / 2.0);
            if (rows.r[osum]) rows.r[osum][k] = make_double2((b.x + c.x) / 2.0, (b.y + c.y) / 2.0);
            if (rows.r[odif]) rows.r[odif][k] = make_double2((b.y - c.y) / 2.0, (c.x - b.x) / 2.0);  // (x + yi) / i = y - xi
        } else {
            const double2 x = rows.r[dsum][k], y = rows.r[ddif][k], u = rows.r[osum][k], w = rows.r[odif][k];
            J2 v;
            v.e[0] = cadd(x, y), v.e[3] = csub(x, y);
            v.e[1] = make_double2(u.x - w.y, u.y + w.x);  // u + i w
            v.e[2] = make_double2(u.x + w.y, u.y - w.x);  // u - i w
            jstore(vis + 4 * k, v);
        }
    }
}

// what gc_solve_run and gc_solve_any need of this module: its launches; the four entries of a gain [T][A][2][2] are planes
// a cell apart, all rotated by the phase of [0][0], the off-diagonals left +0.0 in the diagonal modes
struct JcSolve : JcMod {
    static constexpr int BLOCK = 0, RESIDENT = 0, RAISE_BIT = 0;
    static constexpr int64_t LDS_MOST = (int64_t)JC_LDS_A * (8 + JC_SUMS) * 8;
    static constexpr bool PAIR = false;
    static const void *walker() { return reinterpret_cast<const void *>(jones_iter_kernel); }
    static int64_t lds_antennas() { return JC_LDS_A; }
    static GcPlanes planes(const GcCall &c) { return {4, 1, 4, false, c.mode != 0 ? 6u : 0u}; }
    static GcRules rules(const GcCall &c) { return {"jonescal", 2, false, 64, 64, (size_t)c.A * c.T * 64}; }
    static int run(gridhip_ctx *ctx, const GcCall &c) { return gc_solve_run<JcSolve>(ctx, c); }
    static void init(gridhip_ctx *ctx, const GcCall &c, const GcWork &w)
    {
        hipLaunchKernelGGL(jones_init_kernel, grid_for(ctx, c.A * c.T * JC_SUMS), dim3(256), 0, ctx->stream, c.A * c.T, c.warm,
                           c.mode, w.table, w.ever, w.g);
    }
    static void prepare(gridhip_ctx *ctx, const GcCall &c, const GcWork &w)
    {
        hipLaunchKernelGGL(jones_prepare_kernel, w.sgrid, dim3(256), 0, ctx->stream, c.n, c.A, c.T, c.a1, c.a2, c.slot,
                           (const double2 *)c.vis, (const double2 *)c.model_vis, c.wt, w.real, w.key, w.parts);
    }
    static void iter(gridhip_ctx *ctx, const GcCall &c, const GcWork &w, bool lds, dim3 grid, dim3 block, size_t bytes,
                     int64_t per)
    {
        const double2 *V = (const double2 *)c.vis, *M = (const double2 *)c.model_vis;
        if (lds)
            hipLaunchKernelGGL(jones_iter_kernel, grid, block, bytes, ctx->stream, c.n, (int)c.A, per, (const double *)w.real,
                               (const unsigned long long *)w.key, V, M, (const double2 *)w.g, w.table, (const GcState *)w.st);
        else
            hipLaunchKernelGGL(jones_iter_global_kernel, w.sgrid, dim3(256), 0, ctx->stream, c.n, c.A, (const double *)w.real,
                               (const unsigned long long *)w.key, V, M, (const double2 *)w.g, w.table, (const GcState *)w.st);
    }
    static void update(gridhip_ctx *ctx, const GcCall &c, const GcWork &w)
    {
        hipLaunchKernelGGL(jones_update_kernel, dim3(1), dim3(1024), 0, ctx->stream, c.A * c.T, c.mode, c.tol, w.table, w.ever,
                           w.g, w.st);
    }
    static void final(gridhip_ctx *ctx, const GcCall &c, const GcWork &w)
    {
        hipLaunchKernelGGL(jones_chi_kernel, w.sgrid, dim3(256), 0, ctx->stream, c.n, c.A, (const double *)w.real,
                           (const unsigned long long *)w.key, (const double2 *)w.g, (const double2 *)c.vis,
                           (const double2 *)c.model_vis, w.parts);
    }
};

int apply_jones_check(gridhip_ctx *ctx, int64_t n, int64_t A, int64_t T, const int64_t *a1, const int64_t *a2,
                      const int64_t *slot, const double *gains, int inverse, const double *vis_in, const double *wt_in,
                      const double *vis_out, const double *wt_out)
{
    if (n < 0 || A < 2 || T < 1 || (!slot && T != 1) || (n > 0 && (!a1 || !a2 || !vis_in || !vis_out)) || !gains ||
        inverse < 0 || inverse > 1)
        return fail(ctx, GRIDHIP_EINVAL, "apply_jones: bad argument");
    GH_CHECK(shape_check(ctx, "apply_jones", n, A, T, a1, a2, slot));
    const size_t gb = (size_t)A * T * 64, n8 = (size_t)n * 8;
    const Range vo = {vis_out, 8 * n8}, wo = {wt_out, n8};
    if (overlaps_any(vo, {{gains, gb}, {a1, n8}, {a2, n8}, {slot, n8}}) ||
        overlaps_any(wo, {{gains, gb}, {a1, n8}, {a2, n8}, {slot, n8}}))
        return fail(ctx, GRIDHIP_EINVAL, "apply_jones: an output overlaps gains, a1, a2 or slot");
    // in place: vis_out may be vis_in itself and wt_out may be wt_in itself, nothing else
    if (outputs_clash({vo}, {{vis_in, 8 * n8}, {wt_in, n8}}, {{0, 0}}) ||
        outputs_clash({wo}, {{vis_in, 8 * n8}, {wt_in, n8}}, {{0, 1}}))
        return fail(ctx, GRIDHIP_EINVAL, "apply_jones: an output may be its own input, and overlap no other");
    if (overlap(vo.p, vo.bytes, wo.p, wo.bytes)) return fail(ctx, GRIDHIP_EINVAL, "apply_jones: vis_out overlaps wt_out");
    return GRIDHIP_OK;
}

int stokes_check(gridhip_ctx *ctx, int64_t n, int basis, int which, int inverse, const double *vis, const double *stokes)
{
    if (n < 0 || basis < 0 || basis > 1 || inverse < 0 || inverse > 1 || which < 1 || which > 15 ||
        (inverse && which != 15) || (n > 0 && (!vis || !stokes)))
        return fail(ctx, GRIDHIP_EINVAL, "stokes: n >= 0, basis and inverse in 0..1, which in 1..15 (15 for the inverse), "
                                         "vis and stokes");
    if (overlap(vis, (size_t)n * 64, stokes, (size_t)n * 64))
        return fail(ctx, GRIDHIP_EINVAL, "stokes: vis overlaps the Stokes block");
    return GRIDHIP_OK;
}

int apply_jones_any(gridhip_ctx *ctx, bool dev, int64_t n, int64_t A, int64_t T, const int64_t *a1, const int64_t *a2,
                    const int64_t *slot, const double *gains, int inverse, const double *vis_in, const double *wt_in,
                    double *vis_out, double *wt_out)
{
    if (!ctx) return GRIDHIP_EINVAL;
    GH_CHECK(apply_jones_check(ctx, n, A, T, a1, a2, slot, gains, inverse, vis_in, wt_in, vis_out, wt_out));
    GH_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n8 = (size_t)n * 8;
    Staged st(ctx, dev);
    a1 = st.in(a1, n8), a2 = st.in(a2, n8), slot = st.in(slot, n8), gains = st.in(gains, (size_t)A * T * 64);
    vis_out = st.inout(vis_in, vis_out, 8 * n8);
    if (!dev) vis_in = vis_out;  // (the staged visibilities are corrected in place)
    wt_in = st.in(wt_in, n8), wt_out = st.out(wt_out, n8);
    GH_CHECK(st.status());
    if (n > 0) {
        hipLaunchKernelGGL(jones_apply_kernel, grid_for(ctx, n), dim3(256), 0, ctx->stream, n, A, T, a1, a2, slot,
                           (const double2 *)gains, inverse, (const double2 *)vis_in, wt_in, (double2 *)vis_out, wt_out);
        GH_CHECK_HIP(ctx, hipGetLastError());
    }
    return st.finish();
}

// the Stokes block is staged row by row: a row that is not selected gets no block and is not touched
int stokes_any(gridhip_ctx *ctx, bool dev, int64_t n, int basis, int which, int inverse, double *vis, double *stokes)
{
    if (!ctx) return GRIDHIP_EINVAL;
    GH_CHECK(stokes_check(ctx, n, basis, which, inverse, vis, stokes));
    GH_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n16 = (size_t)n * 16;
    Staged st(ctx, dev);
    vis = inverse ? st.out(vis, 4 * n16) : const_cast<double *>(st.in(vis, 4 * n16));
    StokesRows rows;
    for (int r = 0; r < 4; ++r) {
        double *row = (which >> r & 1) && stokes ? stokes + 2 * n * r : nullptr;
        rows.r[r] = (double2 *)(inverse ? const_cast<double *>(st.in(row, n16)) : st.out(row, n16));
    }
    GH_CHECK(st.status());
    if (n > 0) {
        hipLaunchKernelGGL(stokes_kernel, grid_for(ctx, n), dim3(256), 0, ctx->stream, n, basis, inverse, (double2 *)vis,
                           rows);
        GH_CHECK_HIP(ctx, hipGetLastError());
    }
    return st.finish();
}

}  // namespace

}  // namespace gridhip

using namespace gridhip;

extern "C" {

int64_t gridhip_jonescal_lds_antennas(void) { return JC_LDS_A; }

int gridhip_jonescal_dev(gridhip_ctx *ctx, int64_t n, int64_t A, int64_t T, const int64_t *a1, const int64_t *a2,
                         const int64_t *slot, const double *vis, const double *model_vis, const double *wt, int mode,
                         int64_t refant, int warm, int64_t niter, double tol, double *gains, double *stats)
{
    return gc_solve_any<JcSolve>(ctx, true, {n, A, T, 1, a1, a2, slot, vis, model_vis, wt, mode, refant, warm, niter, tol,
                                             gains, stats});
}

int gridhip_jonescal(gridhip_ctx *ctx, int64_t n, int64_t A, int64_t T, const int64_t *a1, const int64_t *a2,
                     const int64_t *slot, const double *vis, const double *model_vis, const double *wt, int mode,
                     int64_t refant, int warm, int64_t niter, double tol, double *gains, double *stats)
{
    return gc_solve_any<JcSolve>(ctx, false, {n, A, T, 1, a1, a2, slot, vis, model_vis, wt, mode, refant, warm, niter, tol,
                                              gains, stats});
}

int gridhip_apply_jones_dev(gridhip_ctx *ctx, int64_t n, int64_t A, int64_t T, const int64_t *a1, const int64_t *a2,
                            const int64_t *slot, const double *gains, int inverse, const double *vis_in,
                            const double *wt_in, double *vis_out, double *wt_out)
{
    return apply_jones_any(ctx, true, n, A, T, a1, a2, slot, gains, inverse, vis_in, wt_in, vis_out, wt_out);
}

int gridhip_apply_jones(gridhip_ctx *ctx, int64_t n, int64_t A, int64_t T, const int64_t *a1, const int64_t *a2,
                        const int64_t *slot, const double *gains, int inverse, const double *vis_in, const double *wt_in,
                        double *vis_out, double *wt_out)
{
    return apply_jones_any(ctx, false, n, A, T, a1, a2, slot, gains, inverse, vis_in, wt_in, vis_out, wt_out);
}

int gridhip_stokes_dev(gridhip_ctx *ctx, int64_t n, int basis, int which, int inverse, double *vis, double *stokes)
{
    return stokes_any(ctx, true, n, basis, which, inverse, vis, stokes);
}

int gridhip_stokes(gridhip_ctx *ctx, int64_t n, int basis, int which, int inverse, double *vis, double *stokes)
{
    return stokes_any(ctx, false, n, basis, which, inverse, vis, stokes);
}

}  // extern "C"
