// oropt_kernels.hip -- Or-opt on MI355X (gfx950), hand-written HIP: one scan of the segment-move neighbourhood, and the descent
// that alternates it with 2-opt (the reference's local_search, algorithms.py:111-132, with relocate_a2a replaced).
//
// The contract is in include/gnngls_hip.h.  A candidate (i, L, rev, j) takes the chain S = t[i .. i+L-1] out of the tour and puts
// it back, forward or reversed, at index j of the shortened tour t'.  The kernel names the landing place by the TOUR EDGE it
// opens instead: edge p = (t[p], t[p+1]) of the unshortened tour, p = j - 1 in front of the chain (p <= i - 2) and p = j - 1 + L
// behind it (p >= i + L).  Then d = t[p], e = t[p+1] whichever side it is, ascending p is ascending j, and
//      delta = ((((-D[a,s1] - D[sL,c]) + D[a,c]) - D[d,e]) + D[d,s1]) + D[sL,e]               (rev = 1: ... + D[d,sL]) + D[s1,e])
// reads tour-edge lengths (a table in LDS: D[a,s1], D[sL,c], D[d,e]), one wave-uniform entry D[a,c], and two entries each of
// the rows of s1 and sL at the columns t[p], t[p+1] -- the matrix is bitwise symmetric (checked in front of the first scan), so
// D[d,s1] is read as D[s1][d]: a wavefront gathers from two or three rows of n doubles that stay in the vector L1.
//
// Work split: wavefronts over i, lanes over p.  All chains that start at i share the row of s1: a lane loads D[s1][t[p]] and
// D[s1][t[p+1]] once and evaluates L = 1, 2, 3 and both orientations from at most six gathered entries.  The j-independent prefix
// (-D[a,s1] - D[sL,c]) + D[a,c] is wave-uniform.  The arg-min is the (delta, key) minimum of gls_common.h with the key
// (i, L, rev, j) in that order, so the parallel result is the sequential scan's first smallest qualifying candidate.  The 2-opt
// scan of the descent is the plain one (wavefronts over i, lanes over j); nothing here is pruned.
//
// One workgroup per instance, one wavefront per 16 nodes (sixteen at most); the tour (two copies: a move is applied from one into
// the other) and the edge-length table live in LDS, D stays in global memory (a TSP200 matrix is 320 KB: L2).  The descent's
// loop applies one move per trip or ends, and ends after max_moves applied moves: no spin-wait, no watchdog, nothing shared
// between workgroups.  NaNs fail every comparison of the acceptance rule, so such an instance stops at once.
//
// Iterated local search (ils_kernel) is that descent inside a loop of double-bridge kicks, all of it in one launch: the accepted
// tour keeps a third LDS buffer of its own while the kicked candidate descends in the ping-pong pair, so accepting a candidate
// is a swap of three pointers and rejecting one costs nothing.  The cut points of a kick come from the caller's uniforms or
// from philox.h; cut points, kick delta, acceptance, the move cap and the symmetry verdict are computed by every thread from
// the same values (kernel arguments, read-only global memory, LDS behind a barrier), so every branch around a barrier is uniform.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "gls_policy.h"
#include "oropt_kernels.h"
#include "philox.h"

#pragma clang fp contract(off)

namespace gnngls {

#include "gls_common.h"

namespace {

#ifndef OROPT_NODES_PER_WAVE
#define OROPT_NODES_PER_WAVE 16        // one wavefront per this many nodes ...
#endif
#ifndef OROPT_MAX_WAVES
#define OROPT_MAX_WAVES 16             // ... and this many wavefronts per instance at most (<= 16: block_reduce_best)
#endif
// (measured, scripts/bench_or_opt.py, the descent from the nearest-neighbour start at max_seg 1 / 3: 64 nodes per wavefront and
// four wavefronts at most took 1.75 / 2.68 ms for 1,024 TSP100 and 3.50 / 5.19 ms for 256 TSP200 instances, 32 and eight 1.04 /
// 1.64 and 2.26 / 3.49 ms, 16 and sixteen 0.97 / 1.52 and 1.56 / 2.52 ms: a scan is a chain of dependent gathers per row, and
// more wavefronts keep more rows in flight)
constexpr int kOrOptWaves = OROPT_MAX_WAVES;

__host__ __device__ inline size_t oropt_r16(size_t x) { return (x + 15) & ~size_t(15); }
// Ctl | edge lengths [n] fp64 | tour [n+1] | tour [n+1]
__host__ __device__ inline size_t oropt_lds(int n) {
    return oropt_r16(sizeof(Ctl)) + oropt_r16((size_t)n * sizeof(double)) + 2 * oropt_r16((size_t)(n + 1) * sizeof(int32_t));
}

// the same and a third tour buffer: iterated local search keeps the accepted tour beside the ping-pong pair
__host__ __device__ inline size_t ils_lds(int n) { return oropt_lds(n) + oropt_r16((size_t)(n + 1) * sizeof(int32_t)); }

// (i, L, rev, j) in enumeration order: i, j <= 1023
__device__ __forceinline__ int or_opt_key(int i, int L, int rev, int j) { return (i << 13) | ((L - 1) << 11) | (rev << 10) | j; }

// tour after the move, as a function of the old tour: t'[:j] + S (or S reversed) + t'[j:], t' = t without S
__device__ __forceinline__ int or_opt_src(int q, int i, int L, int rev, int j) {
    int r;
    if (q < j) {
        r = q;
    } else if (q < j + L) {
        const int o = q - j;
        return i + (rev ? L - 1 - o : o);
    } else {
        r = q - L;
    }
    return r < i ? r : r + L;
}

// every thread's best (delta, key) over its share of the 2-opt neighbourhood (operators.py:32-50: 1 <= i < j <= n-1, j - i >= 2;
// D[a,b] and D[c,d] are tour edges)
__device__ __forceinline__ void scan_two_opt(const int32_t *t, const double *e, const double *c, int n, int wave, int nwaves, int lane,
                                             double &bd, int &bk) {
    for (int i = 1 + wave; i <= n - 3; i += nwaves) {
        const double *ra = c + (size_t)t[i] * n, *rb = c + (size_t)t[i - 1] * n;
        const double eab = e[i - 1];
        for (int j = i + 2 + lane; j <= n - 1; j += kWave) {
            double delta = ra[t[j]] + rb[t[j - 1]];      // operators.py:25-28, left to right
            delta = delta - eab;
            delta = delta - e[j - 1];
            consider<false>(delta, make_key(i, j), bd, bk);
        }
    }
}

// the same over the Or-opt neighbourhood; lanes own the tour edge p that the chain is put into
__device__ __forceinline__ void scan_or_opt(const int32_t *t, const double *e, const double *c, int n, int max_seg, int reverse, int wave,
                                            int nwaves, int lane, double &bd, int &bk) {
    for (int i = 1 + wave; i <= n - 1; i += nwaves) {
        const int lmax = max_seg < n - i ? max_seg : n - i;            // i + L - 1 <= n - 1
        const double *ra = c + (size_t)t[i - 1] * n, *r1 = c + (size_t)t[i] * n, *r2 = r1, *r3 = r1;
        const double nea = -e[i - 1];
        const double pre1 = (nea - e[i]) + ra[t[i + 1]];
        double pre2 = 0.0, pre3 = 0.0;
        if (lmax >= 2) { r2 = c + (size_t)t[i + 1] * n; pre2 = (nea - e[i + 1]) + ra[t[i + 2]]; }
        if (lmax >= 3) { r3 = c + (size_t)t[i + 2] * n; pre3 = (nea - e[i + 2]) + ra[t[i + 3]]; }
        for (int p = lane; p < n; p += kWave) {
            const bool front = p <= i - 2;               // j = p + 1 <= i - 1; behind the chain j = p + 1 - L >= i + 1
            if (!front && p <= i) continue;              // an edge of the chain's own ends, whatever L is
            const bool fwd = !front || p <= i - 3;       // rev == 0 skips j == i - 1 (operators.py:135)
            const int tp = t[p], tq = t[p + 1];
            const double ep = e[p];
            const double x0 = r1[tp], x1 = r1[tq];
            if (fwd) consider<false>(((pre1 - ep) + x0) + x1, or_opt_key(i, 1, 0, front ? p + 1 : p), bd, bk);
            if (lmax >= 2 && (front || p >= i + 2)) {
                const double y0 = r2[tp], y1 = r2[tq];
                const int j = front ? p + 1 : p - 1;
                if (fwd) consider<false>(((pre2 - ep) + x0) + y1, or_opt_key(i, 2, 0, j), bd, bk);
                if (reverse) consider<false>(((pre2 - ep) + y0) + x1, or_opt_key(i, 2, 1, j), bd, bk);
            }
            if (lmax >= 3 && (front || p >= i + 3)) {
                const double z0 = r3[tp], z1 = r3[tq];
                const int j = front ? p + 1 : p - 2;
                if (fwd) consider<false>(((pre3 - ep) + x0) + z1, or_opt_key(i, 3, 0, j), bd, bk);
                if (reverse) consider<false>(((pre3 - ep) + z0) + x1, or_opt_key(i, 3, 1, j), bd, bk);
            }
        }
    }
}

// the moves are defined for symmetric costs only (rows are read as D[s1][d] for D[d][s1]): one pass over the upper triangle
// against the lower one, bit by bit
__device__ __forceinline__ int asymmetric(const double *c, int n, int tid, int nthr) {
    int bad = 0;
    for (int i = 0; i < n - 1; ++i)
        for (int j = i + 1 + tid; j < n; j += nthr)
            bad |= __double_as_longlong(c[(size_t)i * n + j]) != __double_as_longlong(c[(size_t)j * n + i]);
    return __syncthreads_or(bad);
}

__device__ __forceinline__ void edge_lengths(const int32_t *t, const double *c, int n, double *e, int tid, int nthr) {
    for (int p = tid; p < n; p += nthr) e[p] = c[(size_t)t[p] * n + t[p + 1]];
}

struct Carve {
    Ctl *ctl;
    double *e;
    int32_t *ta, *tb, *tc;                               // tc: ils_kernel only (ils_lds)
};
__device__ __forceinline__ Carve carve(unsigned char *smem, int n) {
    Carve k;
    k.ctl = reinterpret_cast<Ctl *>(smem);
    k.e = reinterpret_cast<double *>(smem + oropt_r16(sizeof(Ctl)));
    k.ta = reinterpret_cast<int32_t *>(smem + oropt_r16(sizeof(Ctl)) + oropt_r16((size_t)n * sizeof(double)));
    k.tb = k.ta + oropt_r16((size_t)(n + 1) * sizeof(int32_t)) / sizeof(int32_t);
    k.tc = k.tb + oropt_r16((size_t)(n + 1) * sizeof(int32_t)) / sizeof(int32_t);
    return k;
}

// the descent (algorithms.py:111-132 with relocate_a2a replaced by the Or-opt scan) from the tour in cur, whose edge lengths are
// in e behind a barrier; it leaves the same state.  cur / nxt swap with every move; cost, moves and status carry on from what
// the caller holds (moves counts against max_moves across calls), trace: the cost after move m at trace[m], m < trace_cap.
// Every thread takes the same trips: bd / bk come out of block_reduce_best uniform, the rest is arguments.
__device__ __forceinline__ void descend(int32_t *&cur, int32_t *&nxt, double *e, Ctl *ctl, int &phase, const double *c, int n, int max_seg,
                                        int reverse, int max_moves, int tid, int nthr, int lane, int wave, int nwaves, double &cost,
                                        int &moves, int &status, double *trace, int trace_cap) {
    bool go = true;
    while (go) {                                         // algorithms.py:116-130; every trip applies a move or is the last
        bool improved = false;
        for (int op = 0; op < 2 && go; ++op) {
            double bd = 0.0;
            int bk = kNoKey;
            if (op == 0) scan_two_opt(cur, e, c, n, wave, nwaves, lane, bd, bk);
            else scan_or_opt(cur, e, c, n, max_seg, reverse, wave, nwaves, lane, bd, bk);
            block_reduce_best<false>(ctl, phase, wave, nwaves, lane, bd, bk);
            if (bk == kNoKey) continue;
            if (op == 0) {
                const int i = bk >> 16, j = bk & 0xffff;
                for (int q = tid; q <= n; q += nthr) nxt[q] = cur[two_opt_src(q, i, j)];
            } else {
                const int i = bk >> 13, L = ((bk >> 11) & 3) + 1, rev = (bk >> 10) & 1, j = bk & 1023;
                for (int q = tid; q <= n; q += nthr) nxt[q] = cur[or_opt_src(q, i, L, rev, j)];
            }
            __syncthreads();
            int32_t *x = cur; cur = nxt; nxt = x;
            edge_lengths(cur, c, n, e, tid, nthr);
            cost += bd;                                  // algorithms.py:124
            if (tid == 0 && trace && moves < trace_cap) trace[moves] = cost;
            ++moves;
            improved = true;
            __syncthreads();
            if (moves >= max_moves) { status = kOrOptStatusMoveCap; go = false; }
        }
        if (!improved) go = false;
    }
}

__global__ __launch_bounds__(kWave *kOrOptWaves) void or_opt_best_move_kernel(const int32_t *tour, const double *D, int n, int max_seg,
                                                                              int reverse, double *delta, int32_t *move, int32_t *new_tour) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const Carve k = carve(smem, n);
    const int b = blockIdx.x, tid = threadIdx.x, nthr = blockDim.x;
    const int lane = tid & (kWave - 1), wave = tid / kWave, nwaves = nthr / kWave;
    const double *c = D + (size_t)b * n * n;
    const int32_t *tin = tour + (size_t)b * (n + 1);
    int32_t *tout = new_tour + (size_t)b * (n + 1);

    for (int q = tid; q <= n; q += nthr) k.ta[q] = tin[q];
    const int bad = asymmetric(c, n, tid, nthr);         // (its barrier also publishes the tour)
    double bd = 0.0;
    int bk = kNoKey;
    if (!bad) {
        edge_lengths(k.ta, c, n, k.e, tid, nthr);
        __syncthreads();
        int phase = 0;
        scan_or_opt(k.ta, k.e, c, n, max_seg, reverse, wave, nwaves, lane, bd, bk);
        block_reduce_best<false>(k.ctl, phase, wave, nwaves, lane, bd, bk);
    }
    const bool none = bk == kNoKey;
    const int i = bk >> 13, L = ((bk >> 11) & 3) + 1, rev = (bk >> 10) & 1, j = bk & 1023;
    for (int q = tid; q <= n; q += nthr) tout[q] = k.ta[none ? q : or_opt_src(q, i, L, rev, j)];
    if (tid == 0) {
        delta[b] = bad ? NAN : bd;
        int32_t *m = move + (size_t)b * 4;
        m[0] = none ? -1 : i; m[1] = none ? -1 : L; m[2] = none ? -1 : rev; m[3] = none ? -1 : j;
    }
}

__global__ __launch_bounds__(kWave *kOrOptWaves) void or_opt_descent_kernel(const int32_t *tour, const double *cost_in, const double *D, int n,
                                                                            int max_seg, int reverse, int max_moves, int32_t *tour_out,
                                                                            double *cost_out, int32_t *moves_out, int32_t *status_out,
                                                                            double *trace_cost, int trace_cap) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const Carve k = carve(smem, n);
    const int b = blockIdx.x, tid = threadIdx.x, nthr = blockDim.x;
    const int lane = tid & (kWave - 1), wave = tid / kWave, nwaves = nthr / kWave;
    const double *c = D + (size_t)b * n * n;
    const int32_t *tin = tour + (size_t)b * (n + 1);
    int32_t *tout = tour_out + (size_t)b * (n + 1);

    int32_t *cur = k.ta, *nxt = k.tb;
    for (int q = tid; q <= n; q += nthr) cur[q] = tin[q];
    double cost = cost_in[b];
    int moves = 0, status = 0;
    if (asymmetric(c, n, tid, nthr)) {                   // (its barrier also publishes the tour)
        status = kOrOptStatusAsymmetric;                 // not searched: the outputs are the inputs
    } else {
        edge_lengths(cur, c, n, k.e, tid, nthr);
        __syncthreads();
        int phase = 0;
        descend(cur, nxt, k.e, k.ctl, phase, c, n, max_seg, reverse, max_moves, tid, nthr, lane, wave, nwaves, cost, moves, status,
                trace_cost ? trace_cost + (size_t)b * trace_cap : nullptr, trace_cap);
    }
    for (int q = tid; q <= n; q += nthr) tout[q] = cur[q];
    if (tid == 0) { cost_out[b] = cost; moves_out[b] = moves; status_out[b] = status; }
}

// min(int(u * k), k - 1), clamped below at 0, k >= 1: one fp64 multiply, truncated.  Every conversion is of a value in
// [0, k); a u outside [0, 1) or a NaN lands on an end of the range
__device__ __forceinline__ int cut_offset(double u, int k) {
    const double x = u * (double)k;
    if (!(x >= 0.0)) return 0;
    return x < (double)k ? (int)x : k - 1;
}

// tour after the orientation-preserving double bridge A D C B, as a function of the old tour: A = t[0:p1], B = t[p1:p2],
// C = t[p2:p3], D = t[p3:n]; position n (the depot) stays
__device__ __forceinline__ int double_bridge_src(int q, int p1, int p2, int p3, int n) {
    if (q < p1 || q >= n) return q;
    const int d_end = p1 + (n - p3), c_end = d_end + (p3 - p2);
    if (q < d_end) return p3 + (q - p1);
    if (q < c_end) return p2 + (q - d_end);
    return p1 + (q - c_end);
}

// iterated local search: descent, then `kicks` times { double bridge on the accepted tour, descent, keep the better tour }
__global__ __launch_bounds__(kWave *kOrOptWaves) void ils_kernel(const int32_t *tour, const double *cost_in, const double *D, int n, int kicks,
                                                                 int kick0, int max_seg, int reverse, int max_moves, uint64_t seed,
                                                                 const double *u, int32_t *tour_out, double *cost_out, int32_t *moves_out,
                                                                 int32_t *accepted_out, int32_t *status_out, double *trace_cost) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const Carve k = carve(smem, n);
    const int b = blockIdx.x, tid = threadIdx.x, nthr = blockDim.x;
    const int lane = tid & (kWave - 1), wave = tid / kWave, nwaves = nthr / kWave;
    const double *c = D + (size_t)b * n * n;
    const int32_t *tin = tour + (size_t)b * (n + 1);
    int32_t *tout = tour_out + (size_t)b * (n + 1);
    const double *ub = u ? u + (size_t)b * kicks * 3 : nullptr;

    int32_t *acc = k.ta, *ping = k.tb, *pong = k.tc;      // the accepted tour, and the pair a candidate descends in
    for (int q = tid; q <= n; q += nthr) acc[q] = tin[q];
    double acc_cost = cost_in[b];
    int moves = 0, status = 0, accepted = 0;
    if (asymmetric(c, n, tid, nthr)) {                   // (its barrier also publishes the tour)
        status = kOrOptStatusAsymmetric;                 // not searched: the outputs are the inputs
    } else {
        edge_lengths(acc, c, n, k.e, tid, nthr);
        __syncthreads();
        int phase = 0;
        descend(acc, ping, k.e, k.ctl, phase, c, n, max_seg, reverse, max_moves, tid, nthr, lane, wave, nwaves, acc_cost, moves, status,
                nullptr, 0);
        const int m = n - 1;
        for (int kick = 0; kick < kicks && status == 0; ++kick) {     // status: uniform (descend), so is every trip
            double u0, u1, u2;
            if (ub) {
                u0 = ub[(size_t)kick * 3]; u1 = ub[(size_t)kick * 3 + 1]; u2 = ub[(size_t)kick * 3 + 2];
            } else {
                const uint32_t kc = (uint32_t)kick0 + (uint32_t)kick;
                u0 = philox_uniform53(seed, (uint32_t)b, kc, 0u, 1u);
                u1 = philox_uniform53(seed, (uint32_t)b, kc, 1u, 1u);
                u2 = philox_uniform53(seed, (uint32_t)b, kc, 2u, 1u);
            }
            const int p1 = 1 + cut_offset(u0, m - 2);                  // 1 .. m-2
            const int p2 = p1 + 1 + cut_offset(u1, m - 1 - p1);        // p1+1 .. m-1
            const int p3 = p2 + 1 + cut_offset(u2, m - p2);            // p2+1 .. m
            __syncthreads();                             // the last scans of the descent before have read ping / pong
            const int ae = acc[p1 - 1], bs = acc[p1], be = acc[p2 - 1], cs = acc[p2], ce = acc[p3 - 1], ds = acc[p3], de = acc[n - 1],
                      z = acc[n];
            double delta = c[(size_t)ae * n + ds] + c[(size_t)de * n + cs];
            delta = delta + c[(size_t)ce * n + bs];
            delta = delta + c[(size_t)be * n + z];
            delta = delta - c[(size_t)ae * n + bs];
            delta = delta - c[(size_t)be * n + cs];
            delta = delta - c[(size_t)ce * n + ds];
            delta = delta - c[(size_t)de * n + z];
            for (int q = tid; q <= n; q += nthr) ping[q] = acc[double_bridge_src(q, p1, p2, p3, n)];
            __syncthreads();
            edge_lengths(ping, c, n, k.e, tid, nthr);
            __syncthreads();
            double cand_cost = acc_cost + delta;
            descend(ping, pong, k.e, k.ctl, phase, c, n, max_seg, reverse, max_moves, tid, nthr, lane, wave, nwaves, cand_cost, moves,
                    status, nullptr, 0);                 // the candidate ends in ping, pong is the free one
            if (tid == 0 && trace_cost) trace_cost[((size_t)b * kicks + kick)] = cand_cost;
            const double d = cand_cost - acc_cost;
            if (d < 0.0 && !close_to_zero(d)) {          // operators.py:42 on the kick; uniform
                int32_t *x = acc; acc = ping; ping = x;
                acc_cost = cand_cost;
                ++accepted;
            }
        }
    }
    for (int q = tid; q <= n; q += nthr) tout[q] = acc[q];
    if (tid == 0) { cost_out[b] = acc_cost; moves_out[b] = moves; accepted_out[b] = accepted; status_out[b] = status; }
}

// ---- guided local search over 2-opt and Or-opt (guided_or_opt_kernel) and the one-to-all scans it is made of -----------------
// The reference's guided_local_search (algorithms.py:135-195) around the descent above: a penalty step picks the tour edge of
// the greatest utility, counts it in the penalty matrix (global memory, int32, both orientations) and runs the one-to-all scans
// of two_opt_o2a and of the Or-opt chains that contain the endpoint on Dg = D + k * penalty.  An entry of Dg is one gather of D,
// one of the penalty, one multiply and one add (contraction is off in this unit: two roundings); the guided lengths of the
// tour's own edges are a second table in LDS beside the plain ones, which the descent and the left-to-right tour cost keep
// reading.  Every scan is a handful of wavefront-sized pieces -- n candidates of 2-opt, at most six chains of n landing edges
// each -- spread over the workgroup and closed by the same arg-min as the all-to-all scans.
struct PlainD {
    const double *c;
    int n;
    __device__ __forceinline__ double operator()(int x, int y) const { return c[x * n + y]; }
};
struct GuidedD {
    const double *c;
    const int32_t *pen;
    double k;
    int n;
    __device__ __forceinline__ double operator()(int x, int y) const {
        const int q = x * n + y;
        const double kp = k * (double)pen[q];            // algorithms.py:164: k * penalty, rounded, then added
        return c[q] + kp;
    }
};

// Ctl | edge lengths [n] | tour | tour | tour (the best one) | guided edge lengths [n] | arg-max slots: 16 x (fp64, int32)
__host__ __device__ inline size_t guided_lds(int n) {
    return ils_lds(n) + oropt_r16((size_t)n * sizeof(double)) + oropt_r16(kOrOptWaves * sizeof(double)) +
           oropt_r16(kOrOptWaves * sizeof(int32_t));
}

// two_opt_o2a (operators.py:53-73) at position i, threads over j; eg[p] = the (guided) length of the tour edge at position p
template <class DG>
__device__ __forceinline__ void scan_two_opt_o2a(const int32_t *t, const double *eg, const DG &dg, int n, int i, int tid, int nthr,
                                                 double &bd, int &bk) {
    for (int j = 1 + tid; j <= n - 1; j += nthr) {
        if (j - i < 2 && i - j < 2) continue;
        const int lo = i < j ? i : j, hi = i < j ? j : i;
        double delta = dg(t[lo], t[hi]) + dg(t[lo - 1], t[hi - 1]);      // operators.py:25-28, left to right
        delta = delta - eg[lo - 1];
        delta = delta - eg[hi - 1];
        consider<false>(delta, j, bd, bk);
    }
}

// the Or-opt candidates (s, L, rev, j) whose chain t[s .. s+L-1] holds position i, in the key order of the all-to-all scan.  A
// piece of work is one chain and 64 landing edges p; pieces go round the wavefronts.  Only the chain's own edges are skipped
// (j == s): the rev == 0, j == s - 1 candidate stays, as relocate_o2a (operators.py:106-126) has it
template <class DG>
__device__ __forceinline__ void scan_or_opt_o2a(const int32_t *t, const double *eg, const DG &dg, int n, int i, int max_seg, int reverse,
                                                int wave, int nwaves, int lane, double &bd, int &bk) {
    const int nblk = (n + kWave - 1) / kWave;
    int piece = 0;
    for (int s = i - max_seg + 1 > 1 ? i - max_seg + 1 : 1; s <= i; ++s) {
        for (int L = i - s + 1; L <= max_seg && s + L - 1 <= n - 1; ++L) {
            for (int blk = 0; blk < nblk; ++blk, ++piece) {
                if (piece % nwaves != wave) continue;
                const int p = blk * kWave + lane;
                if (p >= n || (p >= s - 1 && p <= s + L - 1)) continue;
                const int s1 = t[s], sL = t[s + L - 1];
                const double pre = (-eg[s - 1] - eg[s + L - 1]) + dg(t[s - 1], t[s + L]);
                const int j = p <= s - 2 ? p + 1 : p + 1 - L;
                const int tp = t[p], tq = t[p + 1];
                const double head = pre - eg[p];
                consider<false>((head + dg(s1, tp)) + dg(sL, tq), or_opt_key(s, L, 0, j), bd, bk);
                if (reverse && L >= 2) consider<false>((head + dg(sL, tp)) + dg(s1, tq), or_opt_key(s, L, 1, j), bd, bk);
            }
        }
    }
}

// the first greatest (value, position) of the workgroup (algorithms.py:153-159: `util > max_util or max_util_e is None`);
// pos == kNoKey: a thread without a candidate.  sv / sp: one slot per wavefront, reused only behind a barrier of the caller's
__device__ __forceinline__ void block_argmax_first(double *sv, int32_t *sp, int wave, int nwaves, int lane, double &v, int &pos) {
    wave_argmax_first(v, pos);
    if (nwaves == 1) return;
    if (lane == 0) { sv[wave] = v; sp[wave] = pos; }
    __syncthreads();
    v = sv[0]; pos = sp[0];
    for (int w = 1; w < nwaves; ++w) {
        const double ov = sv[w]; const int op = sp[w];
        if (op != kNoKey && (pos == kNoKey || ov > v || (ov == v && op < pos))) { v = ov; pos = op; }
    }
}

__global__ __launch_bounds__(kWave *kOrOptWaves) void or_opt_o2a_kernel(const int32_t *tour, const double *D, const int32_t *pos, int n,
                                                                        int max_seg, int reverse, double *delta, int32_t *move,
                                                                        int32_t *new_tour) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const Carve k = carve(smem, n);
    const int b = blockIdx.x, tid = threadIdx.x, nthr = blockDim.x;
    const int lane = tid & (kWave - 1), wave = tid / kWave, nwaves = nthr / kWave;
    const double *c = D + (size_t)b * n * n;
    const int32_t *tin = tour + (size_t)b * (n + 1);
    int32_t *tout = new_tour + (size_t)b * (n + 1);
    const int i = pos[b];

    for (int q = tid; q <= n; q += nthr) k.ta[q] = tin[q];
    const int bad = asymmetric(c, n, tid, nthr);         // (its barrier also publishes the tour)
    double bd = 0.0;
    int bk = kNoKey;
    if (!bad && i >= 1 && i <= n - 1) {                  // a position outside 1..n-1 has no candidates
        edge_lengths(k.ta, c, n, k.e, tid, nthr);
        __syncthreads();
        int phase = 0;
        scan_or_opt_o2a(k.ta, k.e, PlainD{c, n}, n, i, max_seg, reverse, wave, nwaves, lane, bd, bk);
        block_reduce_best<false>(k.ctl, phase, wave, nwaves, lane, bd, bk);
    }
    const bool none = bk == kNoKey;
    const int s = bk >> 13, L = ((bk >> 11) & 3) + 1, rev = (bk >> 10) & 1, j = bk & 1023;
    for (int q = tid; q <= n; q += nthr) tout[q] = k.ta[none ? q : or_opt_src(q, s, L, rev, j)];
    if (tid == 0) {
        delta[b] = bad ? NAN : bd;
        int32_t *m = move + (size_t)b * 4;
        m[0] = none ? -1 : s; m[1] = none ? -1 : L; m[2] = none ? -1 : rev; m[3] = none ? -1 : j;
    }
}

// guided local search: descent, then `outer_iters` times { penalty steps until perturbation_moves moves are applied, descent,
// keep the better tour }.  Every thread holds the same cost, counters, status and penalised edge (kernel arguments, values out
// of a workgroup reduction, LDS behind a barrier), so every branch around a barrier is uniform.
__global__ __launch_bounds__(kWave *kOrOptWaves) void guided_or_opt_kernel(
    const int32_t *tour, const double *cost_in, const double *D, const double *guides, int G, int B, const double *k_in, int32_t *penalty,
    int n, int outer_iters, int iter0, int perturbation_moves, int max_seg, int reverse, int max_moves, int max_steps, int32_t *tour_out,
    double *cost_out, int32_t *best_tour, double *best_cost_out, int32_t *moves_out, int32_t *steps_out, int32_t *status_out,
    double *trace_cost, int trace_cap, int32_t *trace_len) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const Carve k = carve(smem, n);
    double *eg = reinterpret_cast<double *>(smem + ils_lds(n));
    double *sv = eg + oropt_r16((size_t)n * sizeof(double)) / sizeof(double);
    int32_t *sp = reinterpret_cast<int32_t *>(sv + oropt_r16(kOrOptWaves * sizeof(double)) / sizeof(double));
    const int b = blockIdx.x, tid = threadIdx.x, nthr = blockDim.x;
    const int lane = tid & (kWave - 1), wave = tid / kWave, nwaves = nthr / kWave;
    const double *c = D + (size_t)b * n * n;
    int32_t *pen = penalty + (size_t)b * n * n;
    const int32_t *tin = tour + (size_t)b * (n + 1);
    double *trace = trace_cost ? trace_cost + (size_t)b * trace_cap : nullptr;
    const double kk = k_in[b];
    const GuidedD dg{c, pen, kk, n};

    int32_t *cur = k.ta, *nxt = k.tb, *best = k.tc;
    for (int q = tid; q <= n; q += nthr) cur[q] = best[q] = tin[q];
    double cost = cost_in[b], best_cost = cost;
    int moves = 0, steps = 0, status = 0;
    if (asymmetric(c, n, tid, nthr)) {                   // (its barrier also publishes the tour)
        status = kOrOptStatusAsymmetric;                 // not searched: the outputs are the inputs
    } else {
        edge_lengths(cur, c, n, k.e, tid, nthr);
        __syncthreads();
        int phase = 0;
        descend(cur, nxt, k.e, k.ctl, phase, c, n, max_seg, reverse, max_moves, tid, nthr, lane, wave, nwaves, cost, moves, status, trace,
                trace_cap);                              // algorithms.py:142
        for (int q = tid; q <= n; q += nthr) best[q] = cur[q];           // :143
        best_cost = cost;
        for (int it = 0; it < outer_iters && status == 0; ++it) {
            const double *guide = guides + ((size_t)((iter0 + it) % G) * B + b) * n * n;       // :147
            int moves_it = 0;
            while (moves_it < perturbation_moves && status == 0) {       // :151
                if (steps >= max_steps) { status = kGuidedStatusStepCap; break; }
                ++steps;
                double uv = 0.0;                         // :153-159, the first greatest utility
                int me = kNoKey;
                for (int p = tid; p < n; p += nthr) {
                    const int q = cur[p] * n + cur[p + 1];
                    const double u = guide[q] / (1.0 + (double)pen[q]);
                    if (me == kNoKey || u > uv) { uv = u; me = p; }
                }
                block_argmax_first(sv, sp, wave, nwaves, lane, uv, me);
                if (me < 0 || me >= n) me = 0;           // (utilities that are all NaN)
                const int na = cur[me], nb = cur[me + 1];
                if (tid == 0) {                          // :161; one thread, plain stores
                    pen[na * n + nb] += 1;
                    pen[nb * n + na] += 1;
                }
                __syncthreads();                         // the counters are visible to the workgroup from here
                for (int p = tid; p < n; p += nthr) eg[p] = k.e[p] + kk * (double)pen[cur[p] * n + cur[p + 1]];
                for (int s = 0; s < 2 && status == 0; ++s) {             // :167
                    const int node = s ? nb : na;
                    if (node == cur[0]) continue;        // :168
                    if (tid == 0) k.ctl->flag = 0;       // :169 cur_tour.index(node): the thread that holds it says where
                    __syncthreads();                     // (this barrier also publishes eg)
                    for (int q = 1 + tid; q < n; q += nthr)
                        if (cur[q] == node) k.ctl->flag = q;
                    __syncthreads();
                    const int i = k.ctl->flag;
                    if (i < 1 || i > n - 1) continue;    // (a tour that is no permutation)
                    for (int op = 0; op < 2 && status == 0; ++op) {      // :171
                        double bd = 0.0;
                        int bk = kNoKey;
                        if (op == 0) scan_two_opt_o2a(cur, eg, dg, n, i, tid, nthr, bd, bk);
                        else scan_or_opt_o2a(cur, eg, dg, n, i, max_seg, reverse, wave, nwaves, lane, bd, bk);
                        block_reduce_best<false>(k.ctl, phase, wave, nwaves, lane, bd, bk);
                        if (bk == kNoKey) continue;
                        if (op == 0) {
                            const int lo = i < bk ? i : bk, hi = i < bk ? bk : i;
                            for (int q = tid; q <= n; q += nthr) nxt[q] = cur[two_opt_src(q, lo, hi)];
                        } else {
                            const int s0 = bk >> 13, L = ((bk >> 11) & 3) + 1, rev = (bk >> 10) & 1, j = bk & 1023;
                            for (int q = tid; q <= n; q += nthr) nxt[q] = cur[or_opt_src(q, s0, L, rev, j)];
                        }
                        __syncthreads();                 // the scan's reads of cur / eg are over, the new tour is complete
                        int32_t *x = cur; cur = nxt; nxt = x;
                        for (int p = tid; p < n; p += nthr) {
                            const int q = cur[p] * n + cur[p + 1];
                            const double d = c[q];
                            k.e[p] = d;
                            eg[p] = d + kk * (double)pen[q];
                        }
                        __syncthreads();
                        if (tid == 0) {                  // :176 tour_cost on the real weights, left to right from 0
                            double sum = 0.0;
                            for (int p = 0; p < n; ++p) sum = sum + k.e[p];
                            k.ctl->cost = sum;
                        }
                        __syncthreads();
                        cost = k.ctl->cost;
                        if (tid == 0 && trace && moves < trace_cap) trace[moves] = cost;
                        ++moves;
                        ++moves_it;                      // :185
                        if (moves >= max_moves) status = kOrOptStatusMoveCap;
                    }
                }
                __syncthreads();                         // the last scans and searches of this step are over
            }
            if (status == 0)                             // :188
                descend(cur, nxt, k.e, k.ctl, phase, c, n, max_seg, reverse, max_moves, tid, nthr, lane, wave, nwaves, cost, moves, status,
                        trace, trace_cap);
            if (cost < best_cost) {                      // :190-191, also for a run a cap has ended
                for (int q = tid; q <= n; q += nthr) best[q] = cur[q];
                best_cost = cost;
            }
        }
    }
    __syncthreads();
    int32_t *tout = tour_out + (size_t)b * (n + 1), *bout = best_tour + (size_t)b * (n + 1);
    for (int q = tid; q <= n; q += nthr) { tout[q] = cur[q]; bout[q] = best[q]; }
    if (tid == 0) {
        cost_out[b] = cost; best_cost_out[b] = best_cost; moves_out[b] = moves; steps_out[b] = steps; status_out[b] = status;
        if (trace_len) trace_len[b] = moves < trace_cap ? moves : trace_cap;
    }
}

}  // namespace

int or_opt_threads(int n) {
    const int waves = (n + OROPT_NODES_PER_WAVE - 1) / OROPT_NODES_PER_WAVE;
    return kWave * (waves < kOrOptWaves ? waves : kOrOptWaves);
}

int or_opt_lds_bytes(int n) { return (int)oropt_lds(n); }

hipError_t launch_or_opt_best_move(const int32_t *tour, const double *D, int B, int n, int max_seg, int reverse, double *delta,
                                   int32_t *move, int32_t *new_tour, hipStream_t stream) {
    static_assert(kOrOptMaxN <= 1024 && kOrOptMaxSeg <= 4, "i and j take ten bits of the selection key, L - 1 two");
    (void)hipGetLastError();
    hipLaunchKernelGGL(or_opt_best_move_kernel, dim3(B), dim3(or_opt_threads(n)), oropt_lds(n), stream, tour, D, n, max_seg, reverse ? 1 : 0,
                       delta, move, new_tour);
    return hipGetLastError();
}

hipError_t launch_or_opt_descent(const int32_t *tour, const double *cost, const double *D, int B, int n, int max_seg, int reverse,
                                 int max_moves, int32_t *tour_out, double *cost_out, int32_t *moves, int32_t *status,
                                 double *trace_cost, int trace_cap, hipStream_t stream) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(or_opt_descent_kernel, dim3(B), dim3(or_opt_threads(n)), oropt_lds(n), stream, tour, cost, D, n, max_seg,
                       reverse ? 1 : 0, max_moves, tour_out, cost_out, moves, status, trace_cost, trace_cap);
    return hipGetLastError();
}

hipError_t launch_ils(const int32_t *tour, const double *cost, const double *D, int B, int n, int kicks, int kick0, int max_seg, int reverse,
                      int max_moves, uint64_t seed, const double *u, int32_t *tour_out, double *cost_out, int32_t *moves,
                      int32_t *accepted, int32_t *status, double *trace_cost, hipStream_t stream) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(ils_kernel, dim3(B), dim3(or_opt_threads(n)), ils_lds(n), stream, tour, cost, D, n, kicks, kick0, max_seg,
                       reverse ? 1 : 0, max_moves, seed, u, tour_out, cost_out, moves, accepted, status, trace_cost);
    return hipGetLastError();
}

hipError_t launch_or_opt_o2a(const int32_t *tour, const double *D, const int32_t *pos, int B, int n, int max_seg, int reverse,
                             double *delta, int32_t *move, int32_t *new_tour, hipStream_t stream) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(or_opt_o2a_kernel, dim3(B), dim3(or_opt_threads(n)), oropt_lds(n), stream, tour, D, pos, n, max_seg, reverse ? 1 : 0,
                       delta, move, new_tour);
    return hipGetLastError();
}

int guided_or_opt_lds_bytes(int n) { return (int)guided_lds(n); }

hipError_t launch_guided_or_opt(const int32_t *tour, const double *cost, const double *D, const double *guides, int G, const double *k,
                                int32_t *penalty, int B, int n, int outer_iters, int iter0, int perturbation_moves, int max_seg,
                                int reverse, int max_moves, int max_steps, int32_t *tour_out, double *cost_out, int32_t *best_tour,
                                double *best_cost, int32_t *moves, int32_t *steps, int32_t *status, double *trace_cost, int trace_cap,
                                int32_t *trace_len, hipStream_t stream) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(guided_or_opt_kernel, dim3(B), dim3(or_opt_threads(n)), guided_lds(n), stream, tour, cost, D, guides, G, B, k,
                       penalty, n, outer_iters, iter0, perturbation_moves, max_seg, reverse ? 1 : 0, max_moves, max_steps, tour_out,
                       cost_out, best_tour, best_cost, moves, steps, status, trace_cost, trace_cap, trace_len);
    return hipGetLastError();
}

}  // namespace gnngls
