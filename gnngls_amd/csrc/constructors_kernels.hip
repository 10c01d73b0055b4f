// constructors_kernels.hip -- the insertion tour constructors on MI355X (gfx950), hand-written HIP.
//
// Replaces (reference file:line, gnngls/...):
//   algorithms.py:82-108   insertion (modes nearest / farthest; mode random with the node order drawn by the host)
//   algorithms.py:67-79    cheapest_insertion            __init__.py:17-21  tour_cost of every candidate tour
//
// One workgroup per instance, the whole construction in one launch.  The tour, its edge weights and their left-to-right prefix
// sums live in LDS; the weight matrix is read from global memory (a step touches two gathers of O(n) entries and one row).
//
// [exact] cheapest_insertion compares tour_cost of the candidate tours, and tour_cost is `c = 0; c += w` edge by edge.  fp64
// addition does not associate, so the candidate at position j is pre[j-1] + W[t[j-1],v] + W[v,t[j]] + ew[j] + ... + ew[L-2]
// added in exactly this order (pre = the prefix sums of the old tour, shared by all candidates): a chain of L-j dependent adds.
// A lane takes the candidates c and L-c, so every lane of a step carries about L adds and the wavefront's lanes finish together;
// the chain's operands come from LDS, where they were staged once, and do not depend on the running sum.  The winner's running
// sums are the next tour's prefix sums; one lane redoes that chain while the others update the node-choice state.
// [exact] node choice (algorithms.py:93-103): `for i in tour: for j in nodes` with a strict compare keeps the first extreme
// pair, i.e. the extreme W[i,j] with ties to the smallest tour position of i, then the smallest j.  Kept incrementally: per
// outside node its extreme weight over the tour members and the member of smallest position that attains it.  An insertion
// shifts later members but keeps their order, so only the new member has to be compared (equal weight: the smaller position).
// Weights must be finite; with NaN the tours are unspecified (but every index stays in range).
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include <type_traits>

#include "constructors_kernels.h"
#include "gls_policy.h"

#pragma clang fp contract(off)

namespace gnngls {

#include "gls_common.h"

namespace {

struct InsLds {
    Ctl *ctl;
    double *pre;        // [m+2] pre[k] = left-to-right sum of the first k edge weights of the tour
    double *ew[2];      // [m+1] ew[p] = W[t[p], t[p+1]] (ping-pong with the tour)
    double *ext;        // [m]   per outside node: extreme weight to a tour member
    int32_t *t[2];      // [m+2] the closed tour
    int32_t *mem;       // [m]   the member of smallest tour position that attains ext
    int32_t *pos;       // [m]   tour position of a node (depot: 0), -1 = outside
};

__host__ __device__ inline size_t ins_r16(size_t x) { return (x + 15) & ~size_t(15); }

__host__ __device__ inline size_t ins_carve(unsigned char *base, int m, InsLds *o) {
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t at = off; off += ins_r16(bytes); return at; };
    const size_t ctl = take(sizeof(Ctl));
    const size_t pre = take((size_t)(m + 2) * 8);
    const size_t e0 = take((size_t)(m + 1) * 8), e1 = take((size_t)(m + 1) * 8);
    const size_t ext = take((size_t)m * 8);
    const size_t t0 = take((size_t)(m + 2) * 4), t1 = take((size_t)(m + 2) * 4);
    const size_t mem = take((size_t)m * 4), pos = take((size_t)m * 4);
    if (o) {
        o->ctl = reinterpret_cast<Ctl *>(base + ctl);
        o->pre = reinterpret_cast<double *>(base + pre);
        o->ew[0] = reinterpret_cast<double *>(base + e0); o->ew[1] = reinterpret_cast<double *>(base + e1);
        o->ext = reinterpret_cast<double *>(base + ext);
        o->t[0] = reinterpret_cast<int32_t *>(base + t0); o->t[1] = reinterpret_cast<int32_t *>(base + t1);
        o->mem = reinterpret_cast<int32_t *>(base + mem); o->pos = reinterpret_cast<int32_t *>(base + pos);
    }
    return off;
}

struct Who { int tid, nthr, lane, wave, nwaves; };

// One cheapest_insertion (algorithms.py:67-79) of node v into the closed tour t[0..L-1]: the position j in 1..L-1 whose candidate
// tour has the strictly smallest tour_cost (first j on ties) and that cost; uniform over the workgroup.
__device__ __forceinline__ void cheapest_step(const double *w, int n, const int32_t *t, const double *ew, const double *pre, int L,
                                              int v, Ctl *ctl, int &phase, const Who &me, double &cost, int &j_out) {
    double bd = INFINITY;
    int bk = kNoKey;
    auto candidate = [&](int j) {
        double s = pre[j - 1];
        s += w[(size_t)t[j - 1] * n + v];
        s += w[(size_t)v * n + t[j]];
#pragma unroll 4
        for (int k = j; k <= L - 2; ++k) s += ew[k];
        if (bk == kNoKey || better<false>(s, j, bd, bk)) { bd = s; bk = j; }
    };
    for (int c = 1 + me.tid; 2 * c <= L; c += me.nthr) {
        candidate(c);                      // L - 1 - c adds behind the prefix
        if (L - c != c) candidate(L - c);  // c - 1 adds
    }
    block_reduce_best<false>(ctl, phase, me.wave, me.nwaves, me.lane, bd, bk);
    if (bk == kNoKey) bk = 1;              // NaN weights only: unspecified, but in range
    cost = bd;
    j_out = bk;
}

// pre[k+1] = pre[k] + ew[k] for k = from .. to-1, left to right (one lane).  Four weights are read before their adds: a read
// behind every store would wait for the LDS round trip four times as often.
__device__ __forceinline__ void prefix_chain(double *pre, const double *ew, int from, int to) {
    double s = pre[from];
    int k = from;
    for (; k + 4 <= to; k += 4) {
        const double e0 = ew[k], e1 = ew[k + 1], e2 = ew[k + 2], e3 = ew[k + 3];
        s += e0; pre[k + 1] = s;
        s += e1; pre[k + 2] = s;
        s += e2; pre[k + 3] = s;
        s += e3; pre[k + 4] = s;
    }
    for (; k < to; ++k) { s += ew[k]; pre[k + 1] = s; }
}

// node of the tour after inserting v at position j, by new position p
__device__ __forceinline__ int inserted_at(const int32_t *t, int p, int j, int v) { return p < j ? t[p] : (p == j ? v : t[p - 1]); }

__global__ __launch_bounds__(1024) void insertion_kernel(const double *W, int n, int depot, int mode, const int32_t *order,
                                                         int32_t *tour_out, int32_t *status) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    InsLds S;
    ins_carve(smem, n, &S);
    const int b = blockIdx.x;
    const Who me{(int)threadIdx.x, (int)blockDim.x, (int)threadIdx.x & (kWave - 1), (int)threadIdx.x / kWave, (int)blockDim.x / kWave};
    const double *w = W + (size_t)b * n * n;
    const int32_t *ord = order ? order + (size_t)b * (n - 1) : nullptr;
    const bool given = mode == INSERT_GIVEN_ORDER, farthest = mode == INSERT_FARTHEST;

    if (given) {
        // the row must be a permutation of the non-depot nodes before any entry is used as an index
        for (int j = me.tid; j < n; j += me.nthr) S.pos[j] = 0;
        __syncthreads();
        int bad = 0;
        for (int k = me.tid; k < n - 1; k += me.nthr) {
            const int v = ord[k];
            if (v < 0 || v >= n || v == depot) bad = 1;
            else if (atomicAdd(&S.pos[v], 1) != 0) bad = 1;
        }
        if (__syncthreads_or(bad)) {
            if (me.tid == 0) status[b] = GNNGLS_STATUS_BAD_ORDER_DEV;
            return;
        }
    }
    if (me.tid == 0 && status) status[b] = 0;
    for (int j = me.tid; j < n; j += me.nthr) {
        S.pos[j] = (j == depot) ? 0 : -1;
        S.mem[j] = depot;
        S.ext[j] = given ? 0.0 : w[(size_t)depot * n + j];
    }
    if (me.tid == 0) {
        S.t[0][0] = depot; S.t[0][1] = depot;
        const double e = w[(size_t)depot * n + depot];
        S.ew[0][0] = e;
        S.pre[0] = 0.0; S.pre[1] = 0.0 + e;
    }
    __syncthreads();

    int phase = 0;
    int32_t *t = S.t[0], *tn = S.t[1];                   // ping-pong: the tour and its edge weights, before / after the insertion
    double *ew = S.ew[0], *ewn = S.ew[1];
    for (int L = 2; L <= n; ++L) {                       // L = entries of the closed tour before this insertion
        int v;
        if (given) {
            v = ord[L - 2];
        } else {
            double bd = INFINITY;
            int bk = kNoKey;
            for (int j = me.tid; j < n; j += me.nthr) {
                if (S.pos[j] >= 0) continue;
                const double x = farthest ? -S.ext[j] : S.ext[j];
                const int key = make_key(S.pos[S.mem[j]], j);
                if (bk == kNoKey || better<false>(x, key, bd, bk)) { bd = x; bk = key; }
            }
            block_reduce_best<false>(S.ctl, phase, me.wave, me.nwaves, me.lane, bd, bk);
            v = bk & 0xffff;
            if (bk == kNoKey) {                          // NaN weights only: the lowest outside node
                v = 0;
                while (v < n - 1 && S.pos[v] >= 0) ++v;
            }
        }
        double cost;
        int j;
        cheapest_step(w, n, t, ew, S.pre, L, v, S.ctl, phase, me, cost, j);

        const double a = w[(size_t)t[j - 1] * n + v], c = w[(size_t)v * n + t[j]];
        for (int p = me.tid; p <= L; p += me.nthr) {
            const int x = inserted_at(t, p, j, v);
            tn[p] = x;
            if (p >= j && p < L) S.pos[x] = p;           // p == L is the closing depot (position 0)
        }
        for (int p = me.tid; p < L; p += me.nthr) ewn[p] = p < j - 1 ? ew[p] : (p == j - 1 ? a : (p == j ? c : ew[p - 1]));
        __syncthreads();
        if (!given) {
            // the new member against every outside node's stored extreme: strictly better replaces it, equal weight keeps
            // the member of smaller tour position
            for (int u = me.tid; u < n; u += me.nthr) {
                if (S.pos[u] >= 0) continue;
                const double x = w[(size_t)v * n + u], e = S.ext[u];
                if ((farthest ? x > e : x < e) || (x == e && j < S.pos[S.mem[u]])) { S.ext[u] = x; S.mem[u] = v; }
            }
        }
        if (me.tid == 0 && L < n) prefix_chain(S.pre, ewn, j - 1, L);      // prefix sums of the new tour from the insertion point on
        { int32_t *x = t; t = tn; tn = x; }
        { double *x = ew; ew = ewn; ewn = x; }
        __syncthreads();
    }
    int32_t *out = tour_out + (size_t)b * (n + 1);
    for (int p = me.tid; p <= n; p += me.nthr) out[p] = t[p];
}

__global__ __launch_bounds__(1024) void cheapest_insertion_kernel(const int32_t *sub_tour, int len, const int32_t *node,
                                                                  const double *W, int n, int32_t *tour_out, double *cost_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    InsLds S;
    ins_carve(smem, len, &S);
    const int b = blockIdx.x;
    const Who me{(int)threadIdx.x, (int)blockDim.x, (int)threadIdx.x & (kWave - 1), (int)threadIdx.x / kWave, (int)blockDim.x / kWave};
    const double *w = W + (size_t)b * n * n;
    const int32_t *s = sub_tour + (size_t)b * len;
    int32_t *t = S.t[0];
    double *ew = S.ew[0];
    const int v = node[b];
    int bad = (v < 0 || v >= n);
    for (int p = me.tid; p < len; p += me.nthr) {
        const int x = s[p];
        if (x < 0 || x >= n) bad = 1;
        t[p] = x;
    }
    if (__syncthreads_or(bad)) {
        if (me.tid == 0) cost_out[b] = NAN;
        return;
    }
    for (int p = me.tid; p < len - 1; p += me.nthr) ew[p] = w[(size_t)t[p] * n + t[p + 1]];
    __syncthreads();
    if (me.tid == 0) {
        S.pre[0] = 0.0;                                  // c = 0; c += w (gnngls/__init__.py:18-20)
        prefix_chain(S.pre, ew, 0, len - 1);
    }
    __syncthreads();
    int phase = 0, j;
    double cost;
    cheapest_step(w, n, t, ew, S.pre, len, v, S.ctl, phase, me, cost, j);
    int32_t *out = tour_out + (size_t)b * (len + 1);
    for (int p = me.tid; p <= len; p += me.nthr) out[p] = inserted_at(t, p, j, v);
    if (me.tid == 0) cost_out[b] = cost;
}

int threads_for(int entries) {          // one lane per pair of candidate positions
    int thr = 64 * ((entries / 2 + 63) / 64);
    return thr < 64 ? 64 : (thr > 1024 ? 1024 : thr);
}

size_t insertion_lds_bytes(int m) { return ins_carve(nullptr, m, nullptr); }

}  // namespace

hipError_t launch_insertion(const double *W, int B, int n, int depot, int mode, const int32_t *order, int32_t *tour_out,
                            int32_t *status, hipStream_t stream) {
    const size_t lds = insertion_lds_bytes(n);
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(insertion_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    (void)hipGetLastError();
    hipLaunchKernelGGL(insertion_kernel, dim3(B), dim3(threads_for(n + 1)), lds, stream, W, n, depot, mode, order, tour_out, status);
    return hipGetLastError();
}

hipError_t launch_cheapest_insertion(const int32_t *sub_tour, int len, const int32_t *node, const double *W, int B, int n,
                                     int32_t *tour_out, double *cost_out, hipStream_t stream) {
    const size_t lds = insertion_lds_bytes(len);
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(cheapest_insertion_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    (void)hipGetLastError();
    hipLaunchKernelGGL(cheapest_insertion_kernel, dim3(B), dim3(threads_for(len)), lds, stream, sub_tour, len, node, W, n, tour_out, cost_out);
    return hipGetLastError();
}

}  // namespace gnngls
