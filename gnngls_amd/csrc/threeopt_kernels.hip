// threeopt_kernels.hip -- 3-opt on MI355X (gfx950), hand-written HIP: one exhaustive scan of the segment-reconnection
// neighbourhood, and the descent that alternates it with 2-opt (the reference's local_search, algorithms.py:111-132, with
// relocate_a2a replaced).
//
// The contract is in include/gnngls_hip.h.  A candidate (p1, p2, p3, kind), 0 <= p1 < p2 < p3 <= n-1, removes the tour edges
// (t[p], t[p+1]) at the three positions and reconnects B = t[p1+1..p2] and C = t[p2+1..p3] between the head t[0..p1] and the tail
// t[p3+1..n]: kind 0 = B reversed + C reversed, 1 = C + B, 2 = C reversed + B, 3 = C + B reversed.  With a1 = t[p1], b1 = t[p1+1],
// b2 = t[p2], c1 = t[p2+1], c2 = t[p3], a2 = t[p3+1]
//      delta = ((((x + y) + z) - D[a1,b1]) - D[b2,c1]) - D[c2,a2]
// with (x, y, z) = (D[a1,b2], D[b1,c2], D[c1,a2]) | (D[a1,c1], D[c2,b1], D[b2,a2]) | (D[a1,c2], D[c1,b1], D[b2,a2]) |
// (D[a1,c1], D[c2,b2], D[b1,a2]).  The removed edges come from the tour-edge table in LDS; the nine distinct added entries are
// gathered once per (p1, p2, p3) and all four kinds are evaluated from them.  The matrix is bitwise symmetric (checked in front
// of the first scan), so D[c2,b1] is read as D[b1][c2].
//
// Work split: wavefronts over p1, lanes over the FLATTENED pairs (p2, p3) of that p1 -- lane l starts at pair l and steps by 64,
// carrying (p2, p3) along by row lengths, so that every pass but a p1's last has all 64 lanes live (lanes over p3 alone would
// leave about half of them idle at n = 100).  A p1 has (n-1-p1)(n-2-p1)/2 pairs: the wavefronts take the p1 of a round in
// alternating direction, which evens out the falling row sizes.  The arg-min is the (delta, key) minimum of gls_common.h with the
// key (p1, p2, p3, kind) in that order -- 8 + 8 + 8 + 2 bits -- so the parallel result is the sequential scan's first smallest
// qualifying candidate, whatever the work split.  Nothing is pruned: every candidate is evaluated.
//
// Where D lives: up to THREEOPT_LDS_MAX_N nodes as a packed lower triangle in LDS, filled by the symmetry pre-pass (which reads
// every entry anyway); beyond it in global memory / L2, rows of a1 and b1 wave-uniform.  One kernel template, two instantiations.
//
// One workgroup per instance, one wavefront per 4 nodes (sixteen at most: from n = 61 on); the tour (two copies: a move is applied
// from one into the other through three_opt_src / two_opt_src), the edge-length table and a table of row offsets by tour position
// (what the index of a gathered entry needs of its node: a multiply and a shift per entry otherwise) live in LDS.  The descent's
// loop applies one move per trip or ends, and ends after max_moves applied moves: no spin-wait, no watchdog, nothing shared
// between workgroups.  NaNs fail every comparison of the acceptance rule, so such an instance stops at once.  Every branch
// around a barrier is uniform: the arg-min's result and the symmetry verdict come out of LDS behind a barrier, the rest is
// kernel arguments.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "gls_policy.h"
#include "threeopt_kernels.h"

#pragma clang fp contract(off)

namespace gnngls {

#include "gls_common.h"

namespace {

#ifndef THREEOPT_NODES_PER_WAVE
#define THREEOPT_NODES_PER_WAVE 4      // one wavefront per this many nodes ...
#endif
#ifndef THREEOPT_MAX_WAVES
#define THREEOPT_MAX_WAVES 16          // ... and this many wavefronts per instance at most (<= 16: block_reduce_best)
#endif
#ifndef THREEOPT_LDS_MAX_N
#define THREEOPT_LDS_MAX_N 200         // the distance triangle is staged in LDS up to this many nodes (0: never; <= 200: it must fit)
#endif
// (measured, scripts/bench_three_opt.py, one scan / the descent from the nearest-neighbour start, 1,024 TSP100 and 256 TSP200
// instances.  Where D lives, all else as shipped: the triangle in LDS 0.56 / 8.20 ms and 1.22 / 25.8 ms, D in global memory
// (-DTHREEOPT_LDS_MAX_N=0) 1.05 / 14.2 and 2.35 / 53.5 ms: the LDS triangle wins at both sizes, so it is used wherever it fits.
// Wavefronts, measured before the row-offset table went in: 4 nodes per wavefront 0.69 / 10.2 and 1.50 / 32.6 ms, 8 nodes -- 13
// wavefronts at TSP100, 16 at TSP200 -- 0.94 / 12.3 and 1.49 / 32.7, 16 nodes -- 7 and 13 -- 0.82 / 10.3 and 1.78 / 39.7: sixteen
// wavefronts, four per SIMD, are the fastest at both sizes.  The row-offset table took the first layout from 0.69 / 10.1 to
// 0.56 / 8.20 ms and from 1.52 / 32.9 to 1.22 / 25.8 ms: the scan is bound by its vector instructions, a third of them index
// arithmetic)
constexpr int kThreeOptWaves = THREEOPT_MAX_WAVES;
constexpr int kThreeOptLdsMaxN = THREEOPT_LDS_MAX_N;

__host__ __device__ inline size_t topt_r16(size_t x) { return (x + 15) & ~size_t(15); }
__host__ __device__ inline size_t topt_tri_entries(int n) { return (size_t)n * (n - 1) / 2 + 1; }      // + 1: the slot a diagonal read of node n-1 would hit
// Ctl | edge lengths [n] fp64 | tour [n+1] | tour [n+1] | row offsets [n+1] | (tri) packed lower triangle of D, fp64
__host__ __device__ inline size_t topt_lds(int n, bool tri) {
    return topt_r16(sizeof(Ctl)) + topt_r16((size_t)n * sizeof(double)) + 3 * topt_r16((size_t)(n + 1) * sizeof(int32_t)) +
           (tri ? topt_r16(topt_tri_entries(n) * sizeof(double)) : 0);
}
inline bool topt_uses_tri(int n) { return n <= kThreeOptLdsMaxN && topt_lds(n, true) <= kLdsPerCU; }

// Both stores answer D[a,b] from the nodes and their ROW OFFSETS: the scans read a node's offset from a table by tour position
// (built with the edge lengths after every move) instead of computing it per gathered entry -- nine entries per (p1, p2, p3).
// D in global memory, row-major: the first index names the row that is read; the row of node a starts at a * n
struct GlobalD {
    const double *c;
    int n;
    __device__ __forceinline__ int rowoff(int a) const { return a * n; }
    __device__ __forceinline__ double at(int a, int oa, int b, int ob) const { (void)a; (void)ob; return c[(unsigned)(oa + b)]; }
    __device__ __forceinline__ double operator()(int a, int b) const { return at(a, rowoff(a), b, rowoff(b)); }
};
// D as a packed lower triangle without diagonal in LDS (every pair a move evaluation reads is a pair of distinct nodes); the
// row of node a starts at a (a - 1) / 2
struct TriD {
    const double *d;
    __device__ __forceinline__ int rowoff(int a) const { return __mul24(a, a - 1) >> 1; }
    __device__ __forceinline__ double at(int a, int oa, int b, int ob) const { return d[a > b ? oa + b : ob + a]; }
    __device__ __forceinline__ double operator()(int a, int b) const { return at(a, rowoff(a), b, rowoff(b)); }
};

// (p1, p2, p3, kind) in enumeration order: positions <= 255
__device__ __forceinline__ int three_opt_key(int p1, int p2, int p3, int kind) { return (p1 << 18) | (p2 << 10) | (p3 << 2) | kind; }

// tour after the move, as a function of the old tour: positions p1+1 .. p3 are refilled from B and C, the rest stays
__device__ __forceinline__ int three_opt_src(int q, int p1, int p2, int p3, int kind) {
    if (q <= p1 || q > p3) return q;
    const int o = q - (p1 + 1), lb = p2 - p1, lc = p3 - p2;
    if (kind == 0) return o < lb ? p2 - o : p3 - (o - lb);             // B reversed + C reversed
    if (o < lc) return kind == 2 ? p3 - o : p2 + 1 + o;                // C (kind 2: reversed) first
    return kind == 3 ? p2 - (o - lc) : p1 + 1 + (o - lc);              // then B (kind 3: reversed)
}

// every thread's best (delta, key) over its share of the 2-opt neighbourhood (operators.py:32-50: 1 <= i < j <= n-1, j - i >= 2;
// D[a,b] and D[c,d] are tour edges): the plain scan, wavefronts over i, lanes over j
template <class DS>
__device__ __forceinline__ void scan_two_opt(const int32_t *t, const int32_t *off, const double *e, const DS &ds, int n, int wave, int nwaves,
                                             int lane, double &bd, int &bk) {
    for (int i = 1 + wave; i <= n - 3; i += nwaves) {
        const int a = t[i], b = t[i - 1], oa = off[i], ob = off[i - 1];
        const double eab = e[i - 1];
        for (int j = i + 2 + lane; j <= n - 1; j += kWave) {
            double delta = ds.at(a, oa, t[j], off[j]) + ds.at(b, ob, t[j - 1], off[j - 1]);      // operators.py:25-28, left to right
            delta = delta - eab;
            delta = delta - e[j - 1];
            consider<false>(delta, make_key(i, j), bd, bk);
        }
    }
}

// the same over the 3-opt neighbourhood: wavefronts over p1, lanes over the flattened pairs (p2, p3), p1 < p2 < p3 <= n-1
template <class DS>
__device__ __forceinline__ void scan_three_opt(const int32_t *t, const int32_t *off, const double *e, const DS &ds, int n, int wave, int nwaves,
                                               int lane, double &bd, int &bk) {
    const int last = n - 1;
    for (int base = 0, round = 0; base <= n - 3; base += nwaves, ++round) {
        const int p1 = base + ((round & 1) ? nwaves - 1 - wave : wave);
        if (p1 > n - 3) continue;
        const int a1 = t[p1], b1 = t[p1 + 1], oa1 = off[p1], ob1 = off[p1 + 1];
        const double e1 = e[p1];
        int p2 = p1 + 1, p3 = p1 + 2 + lane;
        while (p3 > last && p2 <= n - 2) { p3 = p3 - last + (p2 + 1); ++p2; }      // into the row of the next p2
        while (p2 <= n - 2) {
            const int b2 = t[p2], c1 = t[p2 + 1], c2 = t[p3], a2 = t[p3 + 1];
            const int ob2 = off[p2], oc1 = off[p2 + 1], oc2 = off[p3], oa2 = off[p3 + 1];
            const double e2 = e[p2], e3 = e[p3];
            const double a1b2 = ds.at(a1, oa1, b2, ob2), a1c1 = ds.at(a1, oa1, c1, oc1), a1c2 = ds.at(a1, oa1, c2, oc2);
            const double b1c1 = ds.at(b1, ob1, c1, oc1), b1c2 = ds.at(b1, ob1, c2, oc2), b1a2 = ds.at(b1, ob1, a2, oa2);
            const double b2c2 = ds.at(b2, ob2, c2, oc2), b2a2 = ds.at(b2, ob2, a2, oa2), c1a2 = ds.at(c1, oc1, a2, oa2);
            const int key = three_opt_key(p1, p2, p3, 0);
            consider<false>(((((a1b2 + b1c2) + c1a2) - e1) - e2) - e3, key, bd, bk);
            consider<false>(((((a1c1 + b1c2) + b2a2) - e1) - e2) - e3, key | 1, bd, bk);
            consider<false>(((((a1c2 + b1c1) + b2a2) - e1) - e2) - e3, key | 2, bd, bk);
            consider<false>(((((a1c1 + b2c2) + b1a2) - e1) - e2) - e3, key | 3, bd, bk);
            p3 += kWave;
            while (p3 > last && p2 <= n - 2) { p3 = p3 - last + (p2 + 1); ++p2; }
        }
    }
}

// the moves are defined for symmetric costs only (rows are read as D[b1][c2] for D[c2][b1]): one pass over the upper triangle
// against the lower one, bit by bit; with TRI it also stages the triangle in LDS
template <bool TRI>
__device__ __forceinline__ int asymmetric_stage(const double *c, int n, double *tri, int tid, int nthr) {
    int bad = 0;
    for (int i = 0; i < n - 1; ++i)
        for (int j = i + 1 + tid; j < n; j += nthr) {
            const double up = c[(size_t)i * n + j];
            bad |= __double_as_longlong(up) != __double_as_longlong(c[(size_t)j * n + i]);
            if (TRI) tri[(j * (j - 1) >> 1) + i] = up;
        }
    if (TRI && tid == 0) tri[topt_tri_entries(n) - 1] = 0.0;
    return __syncthreads_or(bad);
}

// the tables a scan reads by tour position: the length of the tour edge at p, and the row offset of the node at p
template <class DS>
__device__ __forceinline__ void edge_lengths(const int32_t *t, const DS &ds, int n, double *e, int32_t *off, int tid, int nthr) {
    for (int p = tid; p <= n; p += nthr) {
        off[p] = ds.rowoff(t[p]);
        if (p < n) e[p] = ds(t[p], t[p + 1]);
    }
}

struct Carve {
    Ctl *ctl;
    double *e;
    int32_t *ta, *tb, *off;
    double *tri;                                         // the TRI instantiations only (topt_lds)
};
__device__ __forceinline__ Carve carve(unsigned char *smem, int n) {
    Carve k;
    k.ctl = reinterpret_cast<Ctl *>(smem);
    k.e = reinterpret_cast<double *>(smem + topt_r16(sizeof(Ctl)));
    k.ta = reinterpret_cast<int32_t *>(smem + topt_r16(sizeof(Ctl)) + topt_r16((size_t)n * sizeof(double)));
    k.tb = k.ta + topt_r16((size_t)(n + 1) * sizeof(int32_t)) / sizeof(int32_t);
    k.off = k.tb + topt_r16((size_t)(n + 1) * sizeof(int32_t)) / sizeof(int32_t);
    k.tri = reinterpret_cast<double *>(k.off + topt_r16((size_t)(n + 1) * sizeof(int32_t)) / sizeof(int32_t));
    return k;
}

template <bool TRI> struct StoreOf { using type = GlobalD; };
template <> struct StoreOf<true> { using type = TriD; };
template <bool TRI>
__device__ __forceinline__ typename StoreOf<TRI>::type store_of(const double *c, int n, const double *tri) {
    if constexpr (TRI) return TriD{tri};
    else return GlobalD{c, n};
}

template <bool TRI>
__global__ __launch_bounds__(kWave *kThreeOptWaves) void three_opt_best_move_kernel(const int32_t *tour, const double *D, int n, double *delta,
                                                                                   int32_t *move, int32_t *new_tour) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const Carve k = carve(smem, n);
    const int b = blockIdx.x, tid = threadIdx.x, nthr = blockDim.x;
    const int lane = tid & (kWave - 1), wave = tid / kWave, nwaves = nthr / kWave;
    const double *c = D + (size_t)b * n * n;
    const int32_t *tin = tour + (size_t)b * (n + 1);
    int32_t *tout = new_tour + (size_t)b * (n + 1);
    const auto ds = store_of<TRI>(c, n, k.tri);

    for (int q = tid; q <= n; q += nthr) k.ta[q] = tin[q];
    const int bad = asymmetric_stage<TRI>(c, n, k.tri, tid, nthr);       // (its barrier also publishes the tour and the triangle)
    double bd = 0.0;
    int bk = kNoKey;
    if (!bad) {
        edge_lengths(k.ta, ds, n, k.e, k.off, tid, nthr);
        __syncthreads();
        int phase = 0;
        scan_three_opt(k.ta, k.off, k.e, ds, n, wave, nwaves, lane, bd, bk);
        block_reduce_best<false>(k.ctl, phase, wave, nwaves, lane, bd, bk);
    }
    const bool none = bk == kNoKey;
    const int p1 = bk >> 18, p2 = (bk >> 10) & 255, p3 = (bk >> 2) & 255, kind = bk & 3;
    for (int q = tid; q <= n; q += nthr) tout[q] = k.ta[none ? q : three_opt_src(q, p1, p2, p3, kind)];
    if (tid == 0) {
        delta[b] = bad ? NAN : bd;
        int32_t *m = move + (size_t)b * 4;
        m[0] = none ? -1 : p1; m[1] = none ? -1 : p2; m[2] = none ? -1 : p3; m[3] = none ? -1 : kind;
    }
}

// the descent (algorithms.py:111-132 with relocate_a2a replaced by the 3-opt scan).  cur / nxt swap with every move; trace: the
// cost after move m at trace[m], m < trace_cap.  Every thread takes the same trips: bd / bk come out of block_reduce_best
// uniform, the rest is arguments.
template <bool TRI>
__global__ __launch_bounds__(kWave *kThreeOptWaves) void three_opt_descent_kernel(const int32_t *tour, const double *cost_in, const double *D, int n,
                                                                                 int max_moves, int32_t *tour_out, double *cost_out,
                                                                                 int32_t *moves_out, int32_t *status_out, double *trace_cost,
                                                                                 int trace_cap) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const Carve k = carve(smem, n);
    const int b = blockIdx.x, tid = threadIdx.x, nthr = blockDim.x;
    const int lane = tid & (kWave - 1), wave = tid / kWave, nwaves = nthr / kWave;
    const double *c = D + (size_t)b * n * n;
    const int32_t *tin = tour + (size_t)b * (n + 1);
    int32_t *tout = tour_out + (size_t)b * (n + 1);
    double *trace = trace_cost ? trace_cost + (size_t)b * trace_cap : nullptr;
    const auto ds = store_of<TRI>(c, n, k.tri);

    int32_t *cur = k.ta, *nxt = k.tb;
    double *e = k.e;
    for (int q = tid; q <= n; q += nthr) cur[q] = tin[q];
    double cost = cost_in[b];
    int moves = 0, status = 0;
    if (asymmetric_stage<TRI>(c, n, k.tri, tid, nthr)) { // (its barrier also publishes the tour and the triangle)
        status = kThreeOptStatusAsymmetric;              // not searched: the outputs are the inputs
    } else {
        edge_lengths(cur, ds, n, e, k.off, tid, nthr);
        __syncthreads();
        int phase = 0;
        bool go = true;
        while (go) {                                     // algorithms.py:116-130; every trip applies a move or is the last
            bool improved = false;
            for (int op = 0; op < 2 && go; ++op) {
                double bd = 0.0;
                int bk = kNoKey;
                if (op == 0) scan_two_opt(cur, k.off, e, ds, n, wave, nwaves, lane, bd, bk);
                else scan_three_opt(cur, k.off, e, ds, n, wave, nwaves, lane, bd, bk);
                block_reduce_best<false>(k.ctl, phase, wave, nwaves, lane, bd, bk);
                if (bk == kNoKey) continue;
                if (op == 0) {
                    const int i = bk >> 16, j = bk & 0xffff;
                    for (int q = tid; q <= n; q += nthr) nxt[q] = cur[two_opt_src(q, i, j)];
                } else {
                    const int p1 = bk >> 18, p2 = (bk >> 10) & 255, p3 = (bk >> 2) & 255, kind = bk & 3;
                    for (int q = tid; q <= n; q += nthr) nxt[q] = cur[three_opt_src(q, p1, p2, p3, kind)];
                }
                __syncthreads();
                int32_t *x = cur; cur = nxt; nxt = x;
                edge_lengths(cur, ds, n, e, k.off, tid, nthr);
                cost += bd;                              // algorithms.py:124
                if (tid == 0 && trace && moves < trace_cap) trace[moves] = cost;
                ++moves;
                improved = true;
                __syncthreads();
                if (moves >= max_moves) { status = kThreeOptStatusMoveCap; go = false; }
            }
            if (!improved) go = false;
        }
    }
    for (int q = tid; q <= n; q += nthr) tout[q] = cur[q];
    if (tid == 0) { cost_out[b] = cost; moves_out[b] = moves; status_out[b] = status; }
}

}  // namespace

int three_opt_threads(int n) {
    const int waves = (n + THREEOPT_NODES_PER_WAVE - 1) / THREEOPT_NODES_PER_WAVE;
    return kWave * (waves < kThreeOptWaves ? waves : kThreeOptWaves);
}

int three_opt_lds_bytes(int n) { return (int)topt_lds(n, topt_uses_tri(n)); }

int three_opt_lds_max_n() {
    int n = kThreeOptLdsMaxN < kThreeOptMaxN ? kThreeOptLdsMaxN : kThreeOptMaxN;
    while (n >= 3 && !topt_uses_tri(n)) --n;
    return n >= 3 ? n : 0;
}

hipError_t launch_three_opt_best_move(const int32_t *tour, const double *D, int B, int n, double *delta, int32_t *move,
                                      int32_t *new_tour, hipStream_t stream) {
    static_assert(kThreeOptMaxN <= 256, "a position takes eight bits of the selection key");
    const bool tri = topt_uses_tri(n);
    const size_t lds = topt_lds(n, tri);
    auto kern = tri ? three_opt_best_move_kernel<true> : three_opt_best_move_kernel<false>;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    (void)hipGetLastError();
    hipLaunchKernelGGL(kern, dim3(B), dim3(three_opt_threads(n)), lds, stream, tour, D, n, delta, move, new_tour);
    return hipGetLastError();
}

hipError_t launch_three_opt_descent(const int32_t *tour, const double *cost, const double *D, int B, int n, int max_moves,
                                    int32_t *tour_out, double *cost_out, int32_t *moves, int32_t *status, double *trace_cost,
                                    int trace_cap, hipStream_t stream) {
    const bool tri = topt_uses_tri(n);
    const size_t lds = topt_lds(n, tri);
    auto kern = tri ? three_opt_descent_kernel<true> : three_opt_descent_kernel<false>;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    (void)hipGetLastError();
    hipLaunchKernelGGL(kern, dim3(B), dim3(three_opt_threads(n)), lds, stream, tour, cost, D, n, max_moves, tour_out, cost_out, moves,
                       status, trace_cost, trace_cap);
    return hipGetLastError();
}

}  // namespace gnngls
