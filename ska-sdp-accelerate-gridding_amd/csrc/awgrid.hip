// AW-projection gridders: convgrid3 / convgrid4 (src/Gridding.hs:246-396), which produce the same
// grid, and aw_kernel_fn2 / convolve2d (:761-811) that build each visibility's kernel
//     awkern_k = conj( convolve2d( convolve2d(akerns[a1], akerns[a2]), wkerns[wbin, yf, xf] ) ).
//
// The reference evaluates convolve2d with six 32x32 FFTs per visibility inside a sequential
// `awhile`.  Its pad_mid transposes the operands (padder reads `array ! index2 oldx oldy`, :875),
// so convolve2d(a, b) = same_conv(a, b)^T exactly; here that is evaluated directly:
//   1. the antenna-pair product convolve2d(a1, a2) is computed once per pair that occurs;
//   2. visibilities are de-duplicated by KEY = (pair, wbin, yf, xf) with a device hash table (option
//      "aw_cache"; real data repeats a key over the consecutive dumps of a baseline): the kernel of every
//      distinct key is built once, on the fp64 vector ALU (aw_build_kernel);
//   3. the table of distinct kernels feeds the tap-reusing tile gridder (tile_sorted.hip, AW mode): a record's
//      slice is its key's index, runs of equal key reuse their taps from registers.
// Work is done in batches so the kernel table stays bounded; nothing is read back inside a call.
// The same per-batch preparation feeds the gather (awdegrid: the tile kernel's degrid form reads the same table) and
// aw plans, which keep each batch's records, tables and compacted kernel table for many passes.
#include "imaging.h"
#include "tile_common.h"

namespace gridhip {

constexpr uint64_t AW_EMPTY = ~0ull;

// out[x*S + y] = sum_{i,j} a[i][j] * b[y-i+c][x-j+c]   (c = S/2; a, b in LDS)   == same_conv(a,b)^T
__device__ __forceinline__ void conv_same_T(const double2 *a, const double2 *b, int S, double2 *out, bool conj)
{
    const int c = S / 2;
    for (int o = threadIdx.x; o < S * S; o += blockDim.x) {
        const int x = o / S, y = o - x * S;
        double sr = 0.0, si = 0.0;
        const int ilo = max(0, y + c - (S - 1)), ihi = min(S - 1, y + c);
        const int jlo = max(0, x + c - (S - 1)), jhi = min(S - 1, x + c);
        for (int i = ilo; i <= ihi; ++i) {
            const double2 *arow = a + i * S;
            const double2 *brow = b + (y - i + c) * S + (x + c);
            for (int j = jlo; j <= jhi; ++j) {
                const double2 av = arow[j], bv = brow[-j];
                sr += av.x * bv.x - av.y * bv.y;
                si += av.x * bv.y + av.y * bv.x;
            }
        }
        out[o] = make_double2(sr, conj ? -si : si);
    }
}

// ---- 1. antenna pairs that occur -> dense slots (first come first served; nothing depends on the order)
//   slot[p*A+q]: -1 unseen; counters[0] = pairs so far; pairlist[slot] = p*A+q
__global__ void aw_pairs_kernel(int64_t n, int64_t A, const int64_t *__restrict__ a1, const int64_t *__restrict__ a2,
                                int32_t *__restrict__ slot, int32_t *__restrict__ pairlist, int32_t *__restrict__ counters,
                                int32_t cap)
{
    const int lane = threadIdx.x & 63;
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x) {
        const int64_t p = a1[k], q = a2[k];
        int32_t *s = nullptr;
        bool won = false;
        const bool valid = p >= 0 && p < A && q >= 0 && q < A;
        // consecutive samples of a baseline sit in neighbouring lanes: only the first lane of such a run tries the claim
        const int64_t pq = valid ? p * A + q : -1;
        const int64_t prev = __shfl_up(pq, 1);
        if (valid && (lane == 0 || prev != pq)) {
            s = slot + pq;
            // (claimed already: nothing to do; a stale -1 only costs the atomic)
            if (*s == -1) won = atomicCAS(s, -1, -2) == -1;
        }
        // the wave's new pairs are numbered together: one atomic on the counter per wave, not per pair (10^5 atomics
        // on one address were most of this kernel's 0.19 ms)
        const unsigned long long m = __ballot(won);
        if (m) {
            const int leader = __ffsll((long long)m) - 1;
            int base = 0;
            if (lane == leader) base = atomicAdd(&counters[0], __popcll(m));
            base = __shfl(base, leader);
            if (won) {
                const int32_t id = base + __popcll(m & ((1ull << lane) - 1));
                if (id < cap) pairlist[id] = (int32_t)(p * A + q);
                __hip_atomic_store(s, id < cap ? id : -3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
}

// pairk[slot] = convolve2d(akerns[a1], akerns[a2]) for every pair that occurs (one work-group per pair at a time)
__global__ void aw_pair_kernel(int64_t A, int S, const double2 *__restrict__ akerns, const int32_t *__restrict__ pairlist,
                               const int32_t *__restrict__ counters, int32_t cap, double2 *__restrict__ pairk,
                               int32_t *__restrict__ errors)
{
    extern __shared__ double2 sm[];
    const int npairs = min(counters[0], cap);
    double2 *la = sm, *lb = sm + S * S;
    for (int s = blockIdx.x; s < npairs; s += gridDim.x) {
        int64_t pq = pairlist[s];
        if (pq < 0 || pq >= A * A) {  // (cannot happen: aw_pairs_kernel wrote it)
            pq = 0;
            if (threadIdx.x == 0) atomicAdd(errors, 1);
        }
        const int64_t p = pq / A, q = pq - p * A;
        __syncthreads();
        for (int t = threadIdx.x; t < S * S; t += blockDim.x) {
            la[t] = akerns[p * S * S + t];
            lb[t] = akerns[q * S * S + t];
        }
        __syncthreads();
        conv_same_T(la, lb, S, pairk + (size_t)s * S * S, false);
    }
}

// ---- 2. keys.  key = pair slot << 30 | w-kernel slice (wslice < 2^30, pair slot < 2^31).
// cache: insert into an open-addressing table (64-bit CAS); the first to insert a key numbers it.
//   kid[k]  : index of the visibility's kernel in this batch's table, or -1 (dropped: index out of range)
//   ok[k]   : 0 / -1, handed to the binning pre-pass as the "w-plane" of a one-plane table (-1 is dropped and counted)
//   ukey[id]: the key of table entry id;  counters[1] = entries so far
__global__ void aw_keys_kernel(int64_t H, int64_t Wd, int64_t n, int64_t W, int32_t Q, int64_t A,
                               const double *__restrict__ u, const double *__restrict__ v, int64_t stride,
                               const int64_t *__restrict__ wbin, const int64_t *__restrict__ a1,
                               const int64_t *__restrict__ a2, const int32_t *__restrict__ slot, int cache,
                               unsigned long long *__restrict__ htab, int32_t *__restrict__ hid, uint32_t hmask,
                               int32_t *__restrict__ kid, int64_t *__restrict__ ok, unsigned long long *__restrict__ ukey,
                               int32_t *__restrict__ counters, int32_t cap)
{
    const int lane = threadIdx.x & 63;
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x) {
        const int64_t wb = wbin[k], p = a1[k], q = a2[k];
        const double pu = u[k * stride], pv = v[k * stride];
        int32_t ps = -1;
        if (p >= 0 && p < A && q >= 0 && q < A) ps = slot[p * A + q];
        // the reference would index out of range; such a visibility contributes nothing and is counted
        const bool bad = wb < 0 || wb >= W || ps < 0 || !(pu == pu) || !(pv == pv);
        int32_t id = -1;
        bool won = false;
        uint32_t hwon = 0;
        unsigned long long kwon = 0;
        unsigned long long key = AW_EMPTY;
        if (!bad) {
            int64_t x, y;
            int32_t xf, yf;
            frac_coord_dev(Wd, Q, pu, &x, &xf);
            frac_coord_dev(H, Q, pv, &y, &yf);
            key = ((unsigned long long)ps << 30) | (unsigned long long)((wb * Q + yf) * Q + xf);
            if (!cache) {
                id = (int32_t)k;
                ukey[k] = key;
            }
        }
        if (cache) {
            // consecutive samples of a baseline mostly share their key and sit in neighbouring lanes: only the first lane
            // of such a run probes the table, the others take its slot (the atomics of this kernel are what it costs)
            const unsigned long long prevkey = __shfl_up(key, 1);
            const bool first = !bad && (lane == 0 || prevkey != key);
            uint32_t h = 0;
            if (first) {
                h = (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> 32) & hmask;
                for (;;) {
                    const unsigned long long cur = __hip_atomic_load(&htab[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (cur == key) break;
                    if (cur == AW_EMPTY) {
                        const unsigned long long old = atomicCAS(&htab[h], AW_EMPTY, key);
                        if (old == AW_EMPTY) {  // ours: numbered below, together with the wave's other new keys
                            won = true;
                            break;
                        }
                        if (old == key) break;
                    }
                    h = (h + 1) & hmask;  // (the table has at least twice as many slots as there are keys)
                }
                hwon = h;
                kwon = key;
            }
            // the run's first lane: the highest lane at or below this one that probed
            const unsigned long long fm = __ballot(first) & ((2ull << lane) - 1);
            const int src = fm ? 63 - __clzll((long long)fm) : lane;
            const uint32_t hrun = (uint32_t)__shfl((int)h, src);
            if (!bad) id = -(int32_t)hrun - 16;  // resolved by aw_kid_kernel once every number has been handed out
        }
        // one atomic on the counter per wave for all of its new keys (3 x 10^5 atomics on one address were most of this
        // kernel's 0.33 ms); nobody waits for hid[] inside this launch
        const unsigned long long m = __ballot(won);
        if (m) {
            const int leader = __ffsll((long long)m) - 1;
            int base = 0;
            if (lane == leader) base = atomicAdd(&counters[1], __popcll(m));
            base = __shfl(base, leader);
            if (won) {
                const int32_t nid = base + __popcll(m & ((1ull << lane) - 1));
                if (nid < cap) ukey[nid] = kwon;
                __hip_atomic_store(&hid[hwon], nid < cap ? nid : -3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        if (bad && !cache) ukey[k] = 0;  // (every table entry is built: give the dropped one's a key that exists)
        kid[k] = id;
        ok[k] = bad ? -1 : 0;
    }
}

// second half of the cached form: hash slot -> number (a separate launch, so that every number is visible)
__global__ void aw_kid_kernel(int64_t n, const int32_t *__restrict__ hid, int32_t *__restrict__ kid, int64_t *__restrict__ ok)
{
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x) {
        const int32_t c = kid[k];
        if (c <= -16) {
            const int32_t id = hid[-(c + 16)];
            kid[k] = id;
            if (id < 0) ok[k] = -1;  // (cannot happen: the table holds as many kernels as the batch has visibilities)
        }
    }
}

// ---- 3. kernels of the distinct keys: table[id] = conj(convolve2d(pairk[pair], wkerns[wslice]))
// generic support: one work-group per key at a time
// Nothing read from memory becomes an address before it is in range (the rule of the tile kernels, tile_common.h):
// a key names a pair slot below `npair` and a w-kernel slice below `nslice`; anything else (a stale or overwritten
// table entry - round 2 saw one abort the process) is brought into range and counted in *errors.
__device__ __forceinline__ void aw_key_operands(unsigned long long key, int64_t npair, int64_t nslice, size_t *ia, size_t *ib,
                                                int *bad)
{
    unsigned long long a = key >> 30, b = key & 0x3fffffffull;
    if (a >= (unsigned long long)npair) {
        a = 0;
        ++*bad;
    }
    if (b >= (unsigned long long)nslice) {
        b = 0;
        ++*bad;
    }
    *ia = (size_t)a;
    *ib = (size_t)b;
}

__global__ void aw_build_generic_kernel(int S, const double2 *__restrict__ wkerns, const double2 *__restrict__ pairk,
                                        const unsigned long long *__restrict__ ukey, const int32_t *__restrict__ counters,
                                        int which, int32_t fixed_count, int32_t cap, double2 *__restrict__ table,
                                        int64_t npair_cap, int64_t nslice, int32_t *__restrict__ errors)
{
    extern __shared__ double2 sm[];
    const int nk = min(which >= 0 ? counters[which] : fixed_count, cap);
    const int64_t npair = min((int64_t)counters[0], npair_cap);
    double2 *la = sm, *lb = sm + S * S;
    for (int id = blockIdx.x; id < nk; id += gridDim.x) {
        size_t ia, ib;
        int bad = 0;
        aw_key_operands(ukey[id], npair, nslice, &ia, &ib, &bad);
        if (bad && threadIdx.x == 0) atomicAdd(errors, bad);
        const double2 *pk = pairk + ia * S * S;
        const double2 *wk = wkerns + ib * S * S;
        __syncthreads();
        for (int t = threadIdx.x; t < S * S; t += blockDim.x) {
            la[t] = pk[t];
            lb[t] = wk[t];
        }
        __syncthreads();
        conv_same_T(la, lb, S, table + (size_t)id * S * S, true);
    }
}

// The staged operands are native two-element vectors, not double2 structs: assigning a struct from global memory is a
// memcpy into the array, and an array that is the target of memcpys and lives across the group loop is left in scratch
// memory by the compiler (seen: 60 scratch stores and 30 scratch loads per group).
typedef double aw_d2 __attribute__((ext_vector_type(2)));

// Requests the operands of kernel id_ of a builder group into sa / sb: which S x S arrays it convolves is brought into
// range before it becomes an address; all of the lane's loads together (a load-store loop would pay the memory latency
// per trip).
template <int S, bool PAIR, int NE>
__device__ __forceinline__ void aw_request_operands(aw_d2 (&sa)[NE], aw_d2 (&sb)[NE], int64_t id_, int nk, int x,
                                                    const double2 *__restrict__ wkerns, const double2 *__restrict__ pairk,
                                                    const unsigned long long *__restrict__ ukey,
                                                    const int32_t *__restrict__ pairlist, int64_t A, int64_t npair,
                                                    int64_t nslice, int32_t *__restrict__ errors)
{
    constexpr int S2 = S * S;
    size_t ia = 0, ib = 0;
    if (id_ < nk) {
        int bad = 0;
        if (PAIR) {
            int64_t pq = pairlist[id_];
            if (pq < 0 || pq >= A * A) {
                pq = 0;
                ++bad;
            }
            ia = (size_t)(pq / A);
            ib = (size_t)(pq - (int64_t)ia * A);
        } else
            aw_key_operands(ukey[id_], npair, nslice, &ia, &ib, &bad);
        if (bad && x == 0) atomicAdd(errors, bad);
    }
    const aw_d2 *pk = reinterpret_cast<const aw_d2 *>(pairk + ia * S2);
    const aw_d2 *wk = reinterpret_cast<const aw_d2 *>(wkerns + ib * S2);
#pragma unroll
    for (int t = 0; t < NE; ++t) {
        const int e = min(x + 16 * t, S2 - 1);
        sa[t] = pk[e];
        sb[t] = wk[e];
    }
}

// Compile-time support, organised for the fp64 vector ALU.  A wave builds four kernels at a time: lane = (kernel q,
// column x), and the lane keeps out[y][x] for all S rows y in registers.  The loop nest is ordered so that one LDS
// read feeds many FMAs: for each column j of the pair kernel the lane fetches the S values a[i][j] (all i) and the
// S values b[r][x + c - j] (all r) - 2 S reads - and then performs the S^2 - c(c+1) products of the pairs (i, r)
// whose output row y = r + i - c exists, four FMAs each, from registers: 30 reads per 169 complex products at
// 15 x 15.  b comes from an LDS copy of the w-kernel slice whose rows are followed by c zeros (row pitch S + c, c
// zeros in front of row 0), so a column index of -c .. S-1+c needs no bounds logic.
// PAIR: the same machine builds the antenna-pair products: entry s = convolve2d(akerns[p], akerns[q]) for
// pairlist[s] = p * A + q (wkerns = pairk = akerns, not conjugated).
// ABL (tuning builds, option "dbg"): 1 = the operands are read from LDS once per group instead of once per column j
// (wrong results: what the loop costs without its LDS reads), 2 = no stores of the results, 4 = the group's operands
// requested at its start, not a group ahead (right results)
template <int S, bool PAIR, int ABL = 0>
__global__ void __launch_bounds__(256) aw_build_kernel(const double2 *__restrict__ wkerns, const double2 *__restrict__ pairk,
                                                       const unsigned long long *__restrict__ ukey,
                                                       const int32_t *__restrict__ pairlist, int64_t A,
                                                       const int32_t *__restrict__ counters, int which, int32_t fixed_count,
                                                       int32_t cap, double2 *__restrict__ table, int64_t npair_cap,
                                                       int64_t nslice, int32_t *__restrict__ errors)
{
    constexpr int C = S / 2, PB = S + C, S2 = S * S, BSZ = C + S * PB;  // padded slice: C zeros, then rows of S values + C zeros
    static_assert(S <= 16, "one 16-lane row per kernel");
    extern __shared__ double2 sm[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // shader clock held during this launch (read-only option "aw_clock_khz"): cycle counter and 100 MHz real-time counter
    // stamped by the first work-group when it starts and when it is done; errors points at scalars[31], the stamps are
    // scalars[96..103]
    long long *stamp = reinterpret_cast<long long *>(errors + (96 - 31));
    if (!PAIR && blockIdx.x == 0 && threadIdx.x == 0) {
        stamp[0] = (long long)__builtin_amdgcn_s_memtime();
        stamp[1] = (long long)__builtin_amdgcn_s_memrealtime();
    }
    const int q = lane >> 4, x = lane & 15;
    double2 *abuf = sm + (size_t)(wave * 4 + q) * (S2 + BSZ);  // this kernel's pair kernel ...
    double2 *bbuf = abuf + S2;                                  // ... and padded w-kernel slice
    const int nk = min(which >= 0 ? counters[which] : fixed_count, cap);
    // the zeros of the padded slices are written once
    for (int e = x; e < BSZ; e += 16) {
        const int pos = e - C, col = pos >= 0 ? pos % PB : -1;
        if (pos < 0 || col >= S) bbuf[e] = make_double2(0.0, 0.0);
    }
    const int64_t groups = ((int64_t)nk + 3) / 4, stride = (int64_t)gridDim.x * 4;
    constexpr int NE = (S2 + 15) / 16;
    constexpr bool AHEAD = !(ABL & 4);  // the next group's operands are requested before the current group's products
    aw_d2 sa[NE], sb[NE];
    const int64_t npair = PAIR ? 0 : min((int64_t)counters[0], npair_cap);
#define GH_REQUEST(g_) aw_request_operands<S, PAIR, NE>(sa, sb, (g_) * 4 + q, nk, x, wkerns, pairk, ukey, pairlist, A, npair, nslice, errors)
    int64_t grp = (int64_t)blockIdx.x * 4 + wave;
    if (AHEAD && grp < groups) GH_REQUEST(grp);
    for (; grp < groups; grp += stride) {
        const int64_t id = grp * 4 + q;
        const bool have = id < nk;
        if (!AHEAD) GH_REQUEST(grp);
        __builtin_amdgcn_wave_barrier();  // (the previous group's reads of this LDS region are done: same wave)
#pragma unroll
        for (int t = 0; t < NE; ++t) {
            const int e = x + 16 * t;
            if (e < S2) {
                *reinterpret_cast<aw_d2 *>(abuf + e) = sa[t];
                *reinterpret_cast<aw_d2 *>(bbuf + C + (e / S) * PB + (e % S)) = sb[t];
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        // With one wave per SIMD nothing else covers the ~2 us of these loads: they are in flight during the products
        // (120 registers at 15 x 15, which the one wave has: 512 per lane).
        if (AHEAD) GH_REQUEST(grp + stride);  // (past the last group: kernel 0's operands, not used)

        double2 acc[S];
#pragma unroll
        for (int y = 0; y < S; ++y) acc[y] = make_double2(0.0, 0.0);
        const int xc = x < S ? x : S - 1;  // (the 16th lane of a row repeats the 15th: its results are not stored)
        double2 acol[S], bcol[S];
        if (ABL & 1) {
#pragma unroll
            for (int i = 0; i < S; ++i) acol[i] = abuf[i * S];
#pragma unroll
            for (int r = 0; r < S; ++r) bcol[r] = bbuf[C + xc + C + r * PB];
        }
        for (int j = 0; j < S; ++j) {
            const double2 *bp = bbuf + C + (xc + C - j);  // b[r][xc + C - j] = bp[r * PB]
            if (!(ABL & 1)) {
#pragma unroll
                for (int i = 0; i < S; ++i) acol[i] = abuf[i * S + j];
#pragma unroll
                for (int r = 0; r < S; ++r) bcol[r] = bp[r * PB];
            } else
                asm volatile("" : "+v"(acol[0].x), "+v"(bcol[0].x));  // (keeps the loop a loop)
#pragma unroll
            for (int i = 0; i < S; ++i) {
#pragma unroll
                for (int r = 0; r < S; ++r) {
                    const int y = r + i - C;
                    if (y < 0 || y >= S) continue;  // (compile time)
                    acc[y].x = fma(acol[i].x, bcol[r].x, acc[y].x);
                    acc[y].x = fma(-acol[i].y, bcol[r].y, acc[y].x);
                    acc[y].y = fma(acol[i].x, bcol[r].y, acc[y].y);
                    acc[y].y = fma(acol[i].y, bcol[r].x, acc[y].y);
                }
            }
        }
        if (have && x < S && !((ABL & 2) && acc[0].x != 1.2345e300)) {  // out[x * S + y]: the result comes out transposed, and is conjugated
            double2 *out = table + (size_t)id * S2 + (size_t)x * S;
#pragma unroll
            for (int y = 0; y < S; ++y) out[y] = make_double2(acc[y].x, PAIR ? acc[y].y : -acc[y].y);
        }
    }
    if (!PAIR && blockIdx.x == 0 && threadIdx.x == 0) {
        stamp[2] = (long long)__builtin_amdgcn_s_memtime();
        stamp[3] = (long long)__builtin_amdgcn_s_memrealtime();
    }
#undef GH_REQUEST
}

// records come out of the binning pre-pass with kslice = the visibility's index: replace it by its kernel's
__global__ void aw_relabel_kernel(Geom g, RecWord *__restrict__ recs, const int32_t *__restrict__ nrec,
                                  const int32_t *__restrict__ kid, int32_t nvis)
{
    const int n = min(*nrec, g.nrec);
    const RecWord kmask = ((1ull << g.kb) - 1) << g.ob;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const RecWord w = recs[i];
        const uint32_t o = (uint32_t)(w & ((1ull << g.ob) - 1));
        const uint32_t k = o < (uint32_t)nvis ? (uint32_t)max(kid[o], 0) : 0u;
        recs[i] = (w & ~kmask) | ((RecWord)k << g.ob & kmask);
    }
}

// [30] += [0]: the drops of one batch's binning join the call's total, [31] += [2] its internal errors (every batch's
// binning clears [0..2]; the kernel builders count theirs in [31] directly); [28] += the batch's distinct kernels
__global__ void aw_account_kernel(int32_t *__restrict__ scalars, const int32_t *__restrict__ counters, int cache, int32_t m)
{
    scalars[30] += scalars[0];
    scalars[31] += scalars[2];
    scalars[28] += cache ? counters[1] : m;
    scalars[29] += m;
}
__global__ void aw_finish_kernel(int32_t *__restrict__ scalars)
{
    scalars[0] = scalars[30];
    scalars[2] = scalars[31];
}

}  // namespace gridhip

using namespace gridhip;

namespace {
inline bool cache_on(const gridhip_ctx *ctx) { return ctx->opt.aw_cache != 0; }
template <int S, bool PAIR>
int launch_build(gridhip_ctx *ctx, const double2 *wk, const double2 *pairk, const unsigned long long *ukey,
                 const int32_t *pairlist, int64_t A, const int32_t *counters, int which, int32_t fixed, int32_t cap,
                 double2 *table, int64_t npair_cap, int64_t nslice)
{
    constexpr int C = S / 2, PB = S + C, BSZ = C + S * PB;
    const size_t lds = (size_t)16 * (S * S + BSZ) * sizeof(double2);
#ifdef GRIDHIP_TUNING
    if (S == 15 && !PAIR && ctx->opt.dbg >= 1 && ctx->opt.dbg <= 4) {  // ablations of the key builder (1 - 3: wrong results)
#define AW_ABL1(A_)                                                                                                         \
    if (ctx->opt.dbg == A_) {                                                                                               \
        GH_CHECK(raise_lds(ctx, aw_build_kernel<15, false, A_>));                                                           \
        hipLaunchKernelGGL((aw_build_kernel<15, false, A_>), dim3(ctx->num_cu), dim3(256), lds, ctx->stream, wk, pairk, ukey, \
                           pairlist, A, counters, which, fixed, cap, table, npair_cap, nslice, ctx->d_scalars + 31);       \
    }
        AW_ABL1(1) AW_ABL1(2) AW_ABL1(3) AW_ABL1(4)
#undef AW_ABL1
        return GRIDHIP_OK;
    }
#endif
    GH_CHECK(raise_lds(ctx, aw_build_kernel<S, PAIR>));
    // two work-groups per CU where the LDS holds them (supports up to 11 x 11): two waves per SIMD cover each other's
    // LDS and memory latencies - build phase 1.61 -> 1.51 ms at 11 x 11, 1.18 -> 1.09 ms at 9 x 9 (10^6 visibilities)
    const int nwg = ctx->num_cu * (2 * lds <= (size_t)ctx->max_lds ? 2 : 1);
    // one work-group (four waves, one per SIMD) per CU; the loop strides over the entries
    hipLaunchKernelGGL((aw_build_kernel<S, PAIR>), dim3(nwg), dim3(256), lds, ctx->stream, wk, pairk, ukey, pairlist, A,
                       counters, which, fixed, cap, table, npair_cap, nslice, ctx->d_scalars + 31);
    return GRIDHIP_OK;
}
}  // namespace

namespace gridhip {

// What an aw call decides before its batch loop, and where its scratch lies (ctx->aw).
struct AwCall {
    int64_t W = 0, Q = 0, S = 0, A = 0, batch = 0;
    int32_t pair_cap = 0;
    int cache = 0;
    uint32_t hslots = 0;
    int32_t *slot = nullptr, *pairlist = nullptr, *counters = nullptr, *hid = nullptr, *kid = nullptr;
    double2 *pairk = nullptr, *table = nullptr;  // table: the call scratch's, of batch capacity (null for a plan)
    unsigned long long *htab = nullptr, *ukey = nullptr;
    int64_t *ok = nullptr;
    Prep p;  // geometry of the tile step (one plane: `ok` stands in for wbin; every slice is private to its key)
};

// Limits, then scratch and geometry for n visibilities.  with_table: the call scratch holds a kernel table of batch
// capacity (a plan builds each batch's table in a block of its own, of the batch's distinct count).
static int aw_setup(gridhip_ctx *ctx, int64_t H, int64_t Wd, int64_t n, int64_t W, int64_t Q, int64_t S, int64_t A,
                    bool with_table, AwCall *c)
{
    const size_t S2 = (size_t)S * S, pairs = (size_t)A * A;
    c->W = W;
    c->Q = Q;
    c->S = S;
    c->A = A;
    c->cache = ctx->opt.aw_cache != 0;
    // The table of kernels is sized for the batch whatever the de-duplication finds (nothing is read back inside a
    // call): 2^20 visibilities per batch with the cache (3.8 GB of table at 15 x 15; the 10^6-visibility benchmark is
    // one batch), 2^22 without it, where every visibility has a kernel of its own anyway (15 GB).
    // Option "aw_batch" (> 0) lowers that: fewer visibilities per batch bound the scratch, and let a test run the batch
    // loop at sizes an oracle can follow.
    int64_t bcap = cache_on(ctx) ? ((int64_t)1 << 20) : ((int64_t)1 << 22);
    if (ctx->opt.aw_batch > 0 && ctx->opt.aw_batch < bcap) bcap = ctx->opt.aw_batch;
    c->batch = n < bcap ? n : bcap;
    c->pair_cap = (int32_t)(pairs < (size_t)n ? pairs : (size_t)n);
    c->hslots = 1024;
    while (c->hslots < 2 * (uint64_t)c->batch) c->hslots <<= 1;
    const int64_t batch = c->batch;

    // ---- scratch (grows on first use; laid out in one workspace)
    auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t o_slot = 0, o_plist = o_slot + al(pairs * 4), o_cnt = o_plist + al((size_t)c->pair_cap * 4),
                 o_pairk = o_cnt + al(64), o_htab = o_pairk + al((size_t)c->pair_cap * S2 * 16),
                 o_hid = o_htab + al((size_t)c->hslots * 8), o_kid = o_hid + al((size_t)c->hslots * 4),
                 o_ok = o_kid + al((size_t)batch * 4), o_ukey = o_ok + al((size_t)batch * 8),
                 o_table = o_ukey + al((size_t)batch * 8), total = o_table + (with_table ? al((size_t)batch * S2 * 16) : 0);
    GH_CHECK(ws_reserve(ctx, ctx->aw, total));
    char *base = (char *)ctx->aw.ptr;
    c->slot = (int32_t *)(base + o_slot);
    c->pairlist = (int32_t *)(base + o_plist);
    c->counters = (int32_t *)(base + o_cnt);
    c->pairk = (double2 *)(base + o_pairk);
    c->table = with_table ? (double2 *)(base + o_table) : nullptr;
    c->htab = (unsigned long long *)(base + o_htab);
    c->ukey = (unsigned long long *)(base + o_ukey);
    c->hid = (int32_t *)(base + o_hid);
    c->kid = (int32_t *)(base + o_kid);
    c->ok = (int64_t *)(base + o_ok);

    Prep &p = c->p;
    const int64_t keep_w = ctx->opt.wgroups;
    ctx->opt.wgroups = 1;  // the table is read once per run: nothing for an L2 to keep
    Geom g;
    int block;
    size_t lds;
    int rc = make_geom(ctx, H, Wd, 1, Q, S, S, batch, &g, &block, &lds, 0);  // (no big-tile form of the aw tile kernel)
    ctx->opt.wgroups = keep_w;
    GH_CHECK(rc);
    g.per_vis = 1;
    g.nslices = (int32_t)batch;  // table capacity: a record's kslice is brought below it
    set_rec_bits(&g);
    p.g = g;
    p.block = block;
    p.lds = lds;
    p.nrec = batch;
    p.sorted = ctx->opt.sort != 2 && sorted_plan(ctx, p.g, p.block, &p.nkeys, &p.batch, &p.lds_sorted);
    if (p.sorted) p.g.chunk = p.batch;
    return GRIDHIP_OK;
}

// ---- antenna-pair kernels (once per call)
static int aw_pairs(gridhip_ctx *ctx, const AwCall &c, int64_t n, const double *akerns, const int64_t *a1,
                    const int64_t *a2)
{
    const int64_t A = c.A, S = c.S;
    GH_CHECK_HIP(ctx, hipMemsetAsync(c.slot, 0xff, (size_t)A * A * 4, ctx->stream));
    GH_CHECK_HIP(ctx, hipMemsetAsync(c.counters, 0, 64, ctx->stream));
    int64_t blocks = (n + 255) / 256;
    if (blocks > ctx->num_cu * 8) blocks = ctx->num_cu * 8;
    hipLaunchKernelGGL(aw_pairs_kernel, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, n, A, a1, a2, c.slot, c.pairlist,
                       c.counters, c.pair_cap);
    switch (S) {
#define AW_CASE(S_) \
    case S_: GH_CHECK((launch_build<S_, true>(ctx, (const double2 *)akerns, (const double2 *)akerns, nullptr, c.pairlist, A, c.counters, 0, 0, c.pair_cap, c.pairk, (int64_t)c.pair_cap, (int64_t)A))); break;
        AW_CASE(5) AW_CASE(7) AW_CASE(9) AW_CASE(11) AW_CASE(13) AW_CASE(15)
#undef AW_CASE
        default: {
            int pb = c.pair_cap < ctx->num_cu * 8 ? c.pair_cap : ctx->num_cu * 8;
            hipLaunchKernelGGL(aw_pair_kernel, dim3((unsigned)(pb > 0 ? pb : 1)), dim3(256), 2 * S * S * sizeof(double2), ctx->stream,
                               A, (int)S, (const double2 *)akerns, c.pairlist, c.counters, c.pair_cap, c.pairk, ctx->d_scalars + 31);
        }
    }
    GH_CHECK_HIP(ctx, hipGetLastError());
    return GRIDHIP_OK;
}

// ---- per batch: keys (the batch's visibilities [lo, lo + m); pointers are the call's)
static int aw_keys(gridhip_ctx *ctx, const AwCall &c, int64_t H, int64_t Wd, int64_t lo, int64_t m, const double *u,
                   const double *v, int64_t uv_stride, const int64_t *wbin, const int64_t *a1, const int64_t *a2)
{
    if (c.cache) {
        GH_CHECK_HIP(ctx, hipMemsetAsync(c.htab, 0xff, (size_t)c.hslots * 8, ctx->stream));
        GH_CHECK_HIP(ctx, hipMemsetAsync(c.counters + 1, 0, 4, ctx->stream));
    }
    int64_t kb = (m + 255) / 256;
    if (kb > ctx->num_cu * 8) kb = ctx->num_cu * 8;
    hipLaunchKernelGGL(aw_keys_kernel, dim3((unsigned)kb), dim3(256), 0, ctx->stream, H, Wd, m, c.W, (int32_t)c.Q, c.A,
                       u + lo * uv_stride, v + lo * uv_stride, uv_stride, wbin + lo, a1 + lo, a2 + lo, c.slot, c.cache,
                       c.htab, c.hid, c.hslots - 1, c.kid, c.ok, c.ukey, c.counters, (int32_t)c.batch);
    if (c.cache) hipLaunchKernelGGL(aw_kid_kernel, dim3((unsigned)kb), dim3(256), 0, ctx->stream, m, c.hid, c.kid, c.ok);
    return GRIDHIP_OK;
}

// ---- per batch: the distinct kernels into `table` (entries below the batch's distinct count and `cap` are written)
static int aw_build(gridhip_ctx *ctx, const AwCall &c, int64_t m, const double *wkerns, double2 *table, int64_t cap)
{
    const int which = c.cache ? 1 : -1;
    const int64_t nslice = c.W * c.Q * c.Q;
    switch (c.S) {
#define AW_CASE(S_) \
    case S_: GH_CHECK((launch_build<S_, false>(ctx, (const double2 *)wkerns, c.pairk, c.ukey, nullptr, c.A, c.counters, which, (int32_t)m, (int32_t)cap, table, (int64_t)c.pair_cap, nslice))); break;
        AW_CASE(5) AW_CASE(7) AW_CASE(9) AW_CASE(11) AW_CASE(13) AW_CASE(15)
#undef AW_CASE
        default: {
            int gb = (int)(m < ctx->num_cu * 8 ? m : ctx->num_cu * 8);
            hipLaunchKernelGGL(aw_build_generic_kernel, dim3((unsigned)gb), dim3(256), 2 * c.S * c.S * sizeof(double2), ctx->stream,
                               (int)c.S, (const double2 *)wkerns, c.pairk, c.ukey, c.counters, which, (int32_t)m, (int32_t)cap,
                               table, (int64_t)c.pair_cap, nslice, ctx->d_scalars + 31);
        }
    }
    GH_CHECK_HIP(ctx, hipGetLastError());
    return GRIDHIP_OK;
}

// ---- per batch: binning into ctx->recs / ctx->tables, then each record's kslice becomes its kernel's index.  The
// pre-pass drops the visibilities whose `ok` is -1 (counted); zero_out (degrid): it writes their predictions' zeros.
static int aw_bin(gridhip_ctx *ctx, const AwCall &c, const Geom &g, int64_t lo, int64_t m, const double *u, const double *v,
                  int64_t uv_stride, double *zero_out)
{
    GH_CHECK(launch_bin(ctx, g, m, u + lo * uv_stride, v + lo * uv_stride, uv_stride, c.ok,
                        zero_out ? reinterpret_cast<double2 *>(zero_out + 2 * lo) : nullptr));
    Tables t = tables_of(ctx, g);
    int rb = (int)((m + 255) / 256);
    if (rb > ctx->num_cu * 8) rb = ctx->num_cu * 8;
    hipLaunchKernelGGL(aw_relabel_kernel, dim3((unsigned)rb), dim3(256), 0, ctx->stream, g, (RecWord *)ctx->recs.ptr,
                       t.bin_start + g.nbins, c.kid, (int32_t)m);
    ++ctx->bin_gen;  // (the records are rewritten after their pre-pass)
    return GRIDHIP_OK;
}

// The argument check of the aw entry points: sizes, and the arrays given (has_grid / has_vis: the entry point's grid
// and vis, where it takes them).  A refused call touches nothing.
static int aw_args_ok(gridhip_ctx *ctx, int64_t H, int64_t Wd, int64_t n, int64_t W, int64_t Q, int64_t S, int64_t A,
                      int64_t uv_stride, const double *wkerns, const double *akerns, const double *u, const double *v,
                      const int64_t *wbin, const int64_t *a1, const int64_t *a2, bool has_grid, bool has_vis)
{
    if (!ctx) return GRIDHIP_EINVAL;
    if (H <= 0 || Wd <= 0 || n < 0 || W <= 0 || Q <= 0 || S <= 0 || A <= 0 || uv_stride < 1 || !has_grid || !wkerns ||
        !akerns || (n > 0 && (!u || !v || !wbin || !a1 || !a2 || !has_vis)))
        return fail(ctx, GRIDHIP_EINVAL, "bad argument");
    if (ctx->opt.aw_batch < 0) return fail(ctx, GRIDHIP_EINVAL, "option 'aw_batch' must be >= 0");
    return GRIDHIP_OK;
}

// Start of an aw batch loop or plan: the shapes it takes, then the counters it reports zeroed - [0] dropped, [2] errors,
// [28] distinct kernels built, [29] visibilities keyed, [30] dropped so far (batches), [31] errors so far
static int aw_begin(gridhip_ctx *ctx, int64_t n, int64_t W, int64_t Q, int64_t S, int64_t A)
{
    ctx->aw_tables_built = 0;
    if (S > 63 || A > 46340 || n > (int64_t)0x7fffff00 || W * Q * Q >= ((int64_t)1 << 30))
        return fail(ctx, GRIDHIP_EUNSUPPORTED, "shape outside aw limits");
    GH_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    GH_CHECK_HIP(ctx, hipMemsetAsync(ctx->d_scalars, 0, 4 * sizeof(int32_t), ctx->stream));
    GH_CHECK_HIP(ctx, hipMemsetAsync(ctx->d_scalars + 28, 0, 4 * sizeof(int32_t), ctx->stream));
    return GRIDHIP_OK;
}

// The aw batch loop over one or two (vis, grid) pairs, or (vis_out != null) the gather of one grid into vis_out.  Per
// batch the antenna pairs, keys, the kernel table and the binned records are made once; the tile kernel then runs once
// per pair on the same records and table (it reads ctx->recs and the table, and writes neither).  do_imaging grids its
// baselines twice - image (wt * vis) and PSF (wt) - so its aw form builds the table once where two aw_imaging calls
// would build it twice.  Arguments are checked by the callers; device pointers; asynchronous.
static int aw_batches(gridhip_ctx *ctx, int64_t H, int64_t Wd, int npass, double *const *grids, const double *const *viss,
                      const double *dgrid, double *vis_out, int64_t n, int64_t W, int64_t Q, int64_t S, int64_t A,
                      const double *wkerns, const double *akerns, const double *u, const double *v, int64_t uv_stride,
                      const int64_t *wbin, const int64_t *a1, const int64_t *a2)
{
    GH_CHECK(aw_begin(ctx, n, W, Q, S, A));
    if (n == 0) return GRIDHIP_OK;
    const bool degrid = vis_out != nullptr;
    AwCall c;
    GH_CHECK(aw_setup(ctx, H, Wd, n, W, Q, S, A, true, &c));
    Prep &p = c.p;
    ctx->last_path = p.sorted ? 1 : 3;  // (gridding and the gather alike)
    GH_CHECK(ws_reserve(ctx, ctx->tables, tables_bytes(p.g)));
    GH_CHECK(ws_reserve(ctx, ctx->recs, (size_t)c.batch * sizeof(RecWord)));

    mark(ctx, 0);
    GH_CHECK(aw_pairs(ctx, c, n, akerns, a1, a2));

    // ---- per batch: keys -> distinct kernels -> binning -> tile gridder
    for (int64_t lo = 0; lo < n; lo += c.batch) {
        const int64_t m = n - lo < c.batch ? n - lo : c.batch;
        GH_CHECK(aw_keys(ctx, c, H, Wd, lo, m, u, v, uv_stride, wbin, a1, a2));
        GH_CHECK(aw_build(ctx, c, m, wkerns, c.table, c.batch));
        ++ctx->aw_tables_built;
        mark(ctx, 1);
        p.g.nvis = (int32_t)m;
        p.g.nrec = (int32_t)m;
        GH_CHECK(aw_bin(ctx, c, p.g, lo, m, u, v, uv_stride, vis_out));
        // a pass over the batch's binned records and kernel table: the gather writes the batch's predictions, gridding
        // adds each pair's vis x kernels onto its grid (the tile kernels' errors of every pass land in [2] before the account)
        const double *table = (const double *)c.table;
        if (degrid) GH_CHECK(tile_pass(ctx, p, p.g, m, table, vis_out + 2 * lo, dgrid, true));
        for (int i = 0; i < npass && !degrid; ++i) GH_CHECK(tile_pass(ctx, p, p.g, m, table, viss[i] + 2 * lo, grids[i], false));
        hipLaunchKernelGGL(aw_account_kernel, dim3(1), dim3(1), 0, ctx->stream, ctx->d_scalars, c.counters, c.cache, (int32_t)m);
        mark(ctx, 2);
    }
    hipLaunchKernelGGL(aw_finish_kernel, dim3(1), dim3(1), 0, ctx->stream, ctx->d_scalars);
    GH_CHECK_HIP(ctx, hipGetLastError());
    return GRIDHIP_OK;
}

int awgrid_pairs(gridhip_ctx *ctx, int64_t H, int64_t Wd, int npass, double *const *grids, const double *const *viss,
                 int64_t n, int64_t W, int64_t Q, int64_t S, int64_t A, const double *wkerns, const double *akerns,
                 const double *u, const double *v, int64_t uv_stride, const int64_t *wbin, const int64_t *a1,
                 const int64_t *a2)
{
    return aw_batches(ctx, H, Wd, npass, grids, viss, nullptr, nullptr, n, W, Q, S, A, wkerns, akerns, u, v, uv_stride,
                      wbin, a1, a2);
}

}  // namespace gridhip

// An aw plan: per batch of visibilities its binned records, bin / work tables and the table of its distinct kernels,
// built once; passes lend them to the tile kernels one batch at a time (LendScratch).
struct gridhip_aw_plan {
    gridhip_ctx *ctx = nullptr;
    int64_t n = 0;
    gridhip::Prep p;
    struct Batch {
        int64_t lo = 0, m = 0, nkern = 0;
        gridhip::Workspace recs, tables;
        double2 *table = nullptr;  // nkern distinct kernels
        bool all_binned = false;   // no visibility of the batch was dropped: degrid writes all of its predictions
    };
    std::vector<Batch> b;
    bool caller_clears = false;  // degrid leaves the clearing of its output to the caller (aw_plan_caller_clears)
};

namespace gridhip {
bool aw_plan_caller_clears(gridhip_aw_plan *plan)
{
    plan->caller_clears = true;
    for (const auto &b : plan->b)
        if (!b.all_binned) return true;
    return false;
}
}  // namespace gridhip

namespace {
// the geometry a pass over batch b runs with: its visibilities, and its table's distinct kernels as the slices a
// record's kslice is brought below
gridhip::Geom batch_geom(const gridhip_aw_plan *pl, const gridhip_aw_plan::Batch &b)
{
    gridhip::Geom g = pl->p.g;
    g.nvis = (int32_t)b.m;
    g.nrec = (int32_t)b.m;
    g.nslices = (int32_t)(b.nkern > 0 ? b.nkern : 1);
    return g;
}

// gridding: vis in, grid accumulated; degridding (vis_out != null): grid in, vis_out written
int aw_plan_pass(gridhip_aw_plan *pl, const double *vis, double *grid, double *vis_out)
{
    if (!pl) return GRIDHIP_EINVAL;
    gridhip_ctx *ctx = pl->ctx;
    const bool degrid = vis_out != nullptr;
    if (!grid || (pl->n > 0 && !vis && !vis_out)) return fail(ctx, GRIDHIP_EINVAL, "null pointer");
    GH_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    ctx->aw_tables_built = 0;
    ctx->last_path = pl->p.sorted ? 1 : 3;
    for (auto &b : pl->b) {
        const gridhip::Geom g = batch_geom(pl, b);
        if (degrid && !b.all_binned && !pl->caller_clears)
            GH_CHECK_HIP(ctx, hipMemsetAsync(vis_out + 2 * b.lo, 0, (size_t)b.m * 16, ctx->stream));
        gridhip::LendScratch lend(ctx, b.recs, b.tables);
        GH_CHECK(gridhip::tile_pass(ctx, pl->p, g, b.m, (const double *)b.table, (degrid ? vis_out : vis) + 2 * b.lo, grid,
                                    degrid));
    }
    return GRIDHIP_OK;
}
}  // namespace

extern "C" {

// Device pointers; asynchronous (nothing is read back; scratch grows on first use).
int gridhip_awgrid_dev(gridhip_ctx *ctx, int64_t H, int64_t Wd, double *grid, int64_t n, int64_t W, int64_t Q,
                       int64_t S, int64_t A, const double *wkerns, const double *akerns, const double *u,
                       const double *v, int64_t uv_stride, const int64_t *wbin, const int64_t *a1,
                       const int64_t *a2, const double *vis)
{
    GH_CHECK(aw_args_ok(ctx, H, Wd, n, W, Q, S, A, uv_stride, wkerns, akerns, u, v, wbin, a1, a2, grid, vis));
    return awgrid_pairs(ctx, H, Wd, 1, &grid, &vis, n, W, Q, S, A, wkerns, akerns, u, v, uv_stride, wbin, a1, a2);
}

// What the last gridhip_awgrid*_dev call did (synchronises): visibilities keyed, distinct kernels built.
int gridhip_aw_last_stats(gridhip_ctx *ctx, int64_t *vis_keyed, int64_t *kernels_built)
{
    if (!ctx) return GRIDHIP_EINVAL;
    GH_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    int32_t h[2] = {0, 0};
    GH_CHECK_HIP(ctx, hipMemcpyAsync(h, ctx->d_scalars + 28, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
    GH_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (kernels_built) *kernels_built = h[0];
    if (vis_keyed) *vis_keyed = h[1];
    return GRIDHIP_OK;
}

// Host pointers: convgrid3 / convgrid4 of src/Gridding.hs:246-396 (same result).  Synchronous.
int gridhip_awgrid(gridhip_ctx *ctx, int64_t H, int64_t Wd, double *grid, int64_t n, int64_t W, int64_t Q, int64_t S,
                   int64_t A, const double *wkerns, const double *akerns, const double *u, const double *v,
                   int64_t uv_stride, const int64_t *wbin, const int64_t *a1, const int64_t *a2, const double *vis)
{
    GH_CHECK(aw_args_ok(ctx, H, Wd, n, W, Q, S, A, uv_stride, wkerns, akerns, u, v, wbin, a1, a2, grid, vis));
    GH_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    Staged st(ctx, false);
    grid = st.inout(grid, grid, (size_t)H * Wd * 16);
    u = st.in(u, span_bytes(n, uv_stride)), v = st.in(v, span_bytes(n, uv_stride)), vis = st.in(vis, (size_t)n * 16);
    wbin = st.in(wbin, (size_t)n * 8), wkerns = st.in(wkerns, (size_t)W * Q * Q * S * S * 16);
    akerns = st.in(akerns, (size_t)A * S * S * 16), a1 = st.in(a1, (size_t)n * 8), a2 = st.in(a2, (size_t)n * 8);
    GH_CHECK(st.status());
    GH_CHECK(gridhip_awgrid_dev(ctx, H, Wd, grid, n, W, Q, S, A, wkerns, akerns, u, v, uv_stride, wbin, a1, a2, vis));
    return st.finish();
}

// The gather with convgrid4's coordinates and kernels (include/gridhip.h); device pointers, asynchronous.
int gridhip_awdegrid_dev(gridhip_ctx *ctx, int64_t H, int64_t Wd, const double *grid, int64_t n, int64_t W, int64_t Q,
                         int64_t S, int64_t A, const double *wkerns, const double *akerns, const double *u,
                         const double *v, int64_t uv_stride, const int64_t *wbin, const int64_t *a1,
                         const int64_t *a2, double *vis_out)
{
    GH_CHECK(aw_args_ok(ctx, H, Wd, n, W, Q, S, A, uv_stride, wkerns, akerns, u, v, wbin, a1, a2, grid, vis_out));
    return aw_batches(ctx, H, Wd, 0, nullptr, nullptr, grid, n > 0 ? vis_out : nullptr, n, W, Q, S, A, wkerns, akerns, u,
                      v, uv_stride, wbin, a1, a2);
}

// Host pointers; synchronous.
int gridhip_awdegrid(gridhip_ctx *ctx, int64_t H, int64_t Wd, const double *grid, int64_t n, int64_t W, int64_t Q,
                     int64_t S, int64_t A, const double *wkerns, const double *akerns, const double *u, const double *v,
                     int64_t uv_stride, const int64_t *wbin, const int64_t *a1, const int64_t *a2, double *vis_out)
{
    GH_CHECK(aw_args_ok(ctx, H, Wd, n, W, Q, S, A, uv_stride, wkerns, akerns, u, v, wbin, a1, a2, grid, vis_out));
    GH_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    Staged st(ctx, false);
    grid = st.in(grid, (size_t)H * Wd * 16);
    u = st.in(u, span_bytes(n, uv_stride)), v = st.in(v, span_bytes(n, uv_stride)), vis_out = st.out(vis_out, (size_t)n * 16);
    wbin = st.in(wbin, (size_t)n * 8), wkerns = st.in(wkerns, (size_t)W * Q * Q * S * S * 16);
    akerns = st.in(akerns, (size_t)A * S * S * 16), a1 = st.in(a1, (size_t)n * 8), a2 = st.in(a2, (size_t)n * 8);
    GH_CHECK(st.status());
    GH_CHECK(gridhip_awdegrid_dev(ctx, H, Wd, grid, n, W, Q, S, A, wkerns, akerns, u, v, uv_stride, wbin, a1, a2, vis_out));
    return st.finish();
}

int gridhip_aw_plan_destroy(gridhip_aw_plan *pl)
{
    if (!pl) return GRIDHIP_OK;
    (void)hipSetDevice(pl->ctx->device);
    (void)hipDeviceSynchronize();
    for (auto &b : pl->b) {
        if (b.recs.ptr) (void)hipFree(b.recs.ptr);
        if (b.tables.ptr) (void)hipFree(b.tables.ptr);
        if (b.table) (void)hipFree(b.table);
    }
    delete pl;
    return GRIDHIP_OK;
}

// Per batch: keys, then (synchronising) its distinct count sizes a table of the plan's own, which the builder fills;
// then the binning into blocks of the plan's own.  The inputs are not read after this returns.
int gridhip_aw_plan_create_dev(gridhip_ctx *ctx, int64_t H, int64_t Wd, int64_t n, int64_t W, int64_t Q, int64_t S,
                               int64_t A, const double *wkerns, const double *akerns, const double *u, const double *v,
                               int64_t uv_stride, const int64_t *wbin, const int64_t *a1, const int64_t *a2,
                               gridhip_aw_plan **out)
{
    if (!ctx || !out) return GRIDHIP_EINVAL;
    *out = nullptr;
    GH_CHECK(aw_args_ok(ctx, H, Wd, n, W, Q, S, A, uv_stride, wkerns, akerns, u, v, wbin, a1, a2, true, true));
    GH_CHECK(aw_begin(ctx, n, W, Q, S, A));
    gridhip_aw_plan *pl = new (std::nothrow) gridhip_aw_plan();
    if (!pl) return GRIDHIP_ENOMEM;
    pl->ctx = ctx;
    pl->n = n;
    auto make = [&]() -> int {
        if (n == 0) return GRIDHIP_OK;
        AwCall c;
        GH_CHECK(aw_setup(ctx, H, Wd, n, W, Q, S, A, false, &c));
        pl->p = c.p;
        GH_CHECK(aw_pairs(ctx, c, n, akerns, a1, a2));
        const size_t S2 = (size_t)S * S;
        for (int64_t lo = 0; lo < n; lo += c.batch) {
            const int64_t m = n - lo < c.batch ? n - lo : c.batch;
            pl->b.emplace_back();
            gridhip_aw_plan::Batch &b = pl->b.back();
            b.lo = lo;
            b.m = m;
            GH_CHECK(aw_keys(ctx, c, H, Wd, lo, m, u, v, uv_stride, wbin, a1, a2));
            int32_t nk = (int32_t)m;
            if (c.cache) {
                GH_CHECK_HIP(ctx, hipMemcpyAsync(&nk, c.counters + 1, sizeof nk, hipMemcpyDeviceToHost, ctx->stream));
                GH_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
            }
            b.nkern = nk < 0 ? 0 : nk > m ? m : nk;
            GH_CHECK_HIP(ctx, hipMalloc((void **)&b.table, (size_t)(b.nkern > 0 ? b.nkern : 1) * S2 * 16));
            GH_CHECK(scratch_prefill(ctx, b.table, (size_t)(b.nkern > 0 ? b.nkern : 1) * S2 * 16));
            GH_CHECK(aw_build(ctx, c, m, wkerns, b.table, b.nkern));
            ++ctx->aw_tables_built;
            Geom g = c.p.g;
            g.nvis = (int32_t)m;
            g.nrec = (int32_t)m;
            int32_t binned = 0;
            {
                LendScratch lend(ctx, b.recs, b.tables);
                GH_CHECK(ws_reserve(ctx, ctx->tables, tables_bytes(g)));
                GH_CHECK(ws_reserve(ctx, ctx->recs, (size_t)m * sizeof(RecWord)));
                GH_CHECK(aw_bin(ctx, c, g, lo, m, u, v, uv_stride, nullptr));
                const Tables t = tables_of(ctx, g);
                GH_CHECK_HIP(ctx, hipMemcpyAsync(&binned, t.bin_start + g.nbins, sizeof binned, hipMemcpyDeviceToHost, ctx->stream));
            }
            hipLaunchKernelGGL(aw_account_kernel, dim3(1), dim3(1), 0, ctx->stream, ctx->d_scalars, c.counters, c.cache, (int32_t)m);
            GH_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));  // (the batch's binned count)
            b.all_binned = binned == (int32_t)m && ctx->opt.fault_inject == 0;
        }
        hipLaunchKernelGGL(aw_finish_kernel, dim3(1), dim3(1), 0, ctx->stream, ctx->d_scalars);
        GH_CHECK_HIP(ctx, hipGetLastError());
        // the inputs may be freed or overwritten once this returns
        GH_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return GRIDHIP_OK;
    };
    const int rc = make();
    if (rc != GRIDHIP_OK) {
        gridhip_aw_plan_destroy(pl);
        return rc;
    }
    *out = pl;
    return GRIDHIP_OK;
}

int gridhip_aw_plan_grid_dev(gridhip_aw_plan *plan, const double *vis, double *grid)
{
    return aw_plan_pass(plan, vis, grid, nullptr);
}

int gridhip_aw_plan_degrid_dev(gridhip_aw_plan *plan, const double *grid, double *vis_out)
{
    if (!plan) return GRIDHIP_EINVAL;
    if (plan->n > 0 && !vis_out) return fail(plan->ctx, GRIDHIP_EINVAL, "null pointer");
    if (plan->n == 0) return grid ? GRIDHIP_OK : fail(plan->ctx, GRIDHIP_EINVAL, "null pointer");
    return aw_plan_pass(plan, nullptr, const_cast<double *>(grid), vis_out);
}

}  // extern "C"
