// greedy_edge_kernels.hip -- greedy edge matching ("greedy merge") decoding of tours from any edge score on MI355X (gfx950),
// hand-written HIP.
//
// The reference has no counterpart.  include/gnngls_hip.h states the definition (gnngls_greedy_edge), gnngls_amd.host.greedy_edge
// restates it in NumPy (host.greedy_edge_rounds restates the rounds below) and the device matches both bit for bit.
//
// The definition is sequential -- the n (n - 1) / 2 edges in ascending (key, i, j), n - 1 dependent acceptances -- and is run here
// without a sort and without stored keys, one workgroup of min(ceil(n / 16), 16) wavefronts per instance, one launch per batch.
// Per node, in LDS: its degree, its two tour neighbours, other[u] (the far end of the path fragment u is an end of; a single node
// is both ends of its own) and a cached candidate cand[u] = (key, j): the smallest VALID edge at u in (key, i, j), where {u, j} is
// valid iff deg[u] < 2, deg[j] < 2, j != u and j != other[u].  For a fixed u that order is (key, j): partners below u give edges
// (j, u), which precede the edges (u, j) of partners above u, both in ascending j.
//
//   FIRST.   Every row of S is scanned once, one wavefront per row (coalesced, four pieces of 64 entries in flight), for its arg-min
//            in (key, j) by a butterfly over the 64 lanes -- and for an entry that is not finite, which refuses the instance on a
//            workgroup-uniform flag before the rounds begin.
//   ROUND 1. RESCAN.  Every end node whose cached candidate is no longer valid is appended to a list; one wavefront takes one listed
//            row.  Validity only ever shrinks, so a cached minimum that is still valid is still the minimum.
//         2. DOMINANCE.  e = {u, v} is dominant iff min(cand[u], cand[other[u]]) == e == min(cand[v], cand[other[v]]).  The thread
//            of the smaller end decides: cand[v] names u, and the candidates of the two far ends are larger in (key, i, j).
//         3. ACCEPT.  All dominant edges at once, each by its one thread: degrees, neighbours, other[] of the two far ends.  Two
//            dominant edges never share a fragment, so there is no conflict; the globally smallest valid edge is always dominant, so
//            every round accepts; the loop ends on the workgroup-uniform count n - 1 (DESIGN.md has the exactness argument).
//   CLOSE.   The two nodes of degree 1 are joined.  `edges`, when asked for: the accepted edges ranked by counting in (key, i, j),
//            which IS the acceptance order of the definition.  One thread walks the neighbours from the depot into LDS; all threads
//            gather the tour's keys and lengths; one thread each sums them left to right in fp64.
//
// The kernel reads row u of S for node u, so S has to be bitwise symmetric off the diagonal (ops.greedy_edge checks it).  With a
// matrix that is not, a round may find no dominant edge: the loop then ends on that workgroup-uniform fact and the instance gets
// kGreedyEdgeStatusStalled -- nothing is indexed out of range and nothing spins.
//
// [exact] the only fp64 operations are the adds of the two sums (contraction off); keys are compared as order-preserving uint64.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "greedy_edge_kernels.h"

#pragma clang fp contract(off)

namespace gnngls {

namespace {

constexpr int kLanes = 64;
constexpr int kUnroll = 4;                           // row pieces of 64 entries whose loads are in flight together
constexpr uint64_t kNoKey = ~0ull;                   // above the key of every finite value
constexpr int kNoNode = 0x7FFFFFFF;

struct GreedyCtl {
    int32_t bad, nlist, accepted, e0, e1, pad[3];
};

__host__ __device__ inline size_t ge_r16(size_t x) { return (x + 15) & ~(size_t)15; }

// the value as a uint64 whose unsigned order is the fp64 order (finite values only); -0.0 and +0.0 -> one key
__device__ __forceinline__ uint64_t ord_key(double v) {
    uint64_t b = (uint64_t)__double_as_longlong(v);
    if ((b << 1) == 0ull) b = 0ull;
    return b ^ ((b >> 63) ? ~0ull : 0x8000000000000000ull);
}

// (key, min, max) of the candidate (k, j) cached at node u, against the edge (ek, ei, ej): strictly larger?
__device__ __forceinline__ bool cand_above(uint64_t k, int u, int j, uint64_t ek, int ei, int ej) {
    const int i0 = u < j ? u : j, j0 = u < j ? j : u;
    return k > ek || (k == ek && (i0 > ei || (i0 == ei && j0 > ej)));
}

// The arg-min in (key, j) over the valid partners j of node u (deg[j] < 2, j != u, j != ou), by all lanes of one wavefront: every
// lane ends with the answer, (kNoKey, kNoNode) where there is none.  The loads are unconditional (a select around a load would
// serialise them): a lane beyond n reads column n - 1, and the entries of u itself (the diagonal) and of closed nodes are read
// too, but no such value is ever used.  kCheck: also tells whether an off-diagonal entry of the row is not finite.
template <bool kCheck>
__device__ __forceinline__ void scan_row(const double *row, int n, int u, int ou, const int32_t *deg, int lane, uint64_t &bk, int &bj,
                                         bool &bad) {
    bk = kNoKey;
    bj = kNoNode;
    for (int j0 = 0; j0 < n; j0 += kLanes * kUnroll) {
        double v[kUnroll];
        int jj[kUnroll], dj[kUnroll];
#pragma unroll
        for (int q = 0; q < kUnroll; ++q) {
            jj[q] = j0 + q * kLanes + lane;
            const int jc = jj[q] < n ? jj[q] : n - 1;
            v[q] = row[jc];
            dj[q] = deg[jc];
        }
#pragma unroll
        for (int q = 0; q < kUnroll; ++q) {
            const bool valid = jj[q] < n && jj[q] != u && jj[q] != ou && dj[q] < 2;
            if (kCheck && jj[q] < n && jj[q] != u && !isfinite(v[q])) bad = true;
            const uint64_t k = ord_key(v[q]);
            if (valid && k < bk) { bk = k; bj = jj[q]; }                 // jj ascends in a lane: the first of equal keys stays
        }
    }
#pragma unroll
    for (int d = kLanes / 2; d >= 1; d >>= 1) {
        const uint64_t ok = (uint64_t)__shfl_xor((unsigned long long)bk, d);
        const int oj = __shfl_xor(bj, d);
        if (ok < bk || (ok == bk && oj < bj)) { bk = ok; bj = oj; }
    }
}

__global__ __launch_bounds__(kLanes *kGreedyEdgeMaxWaves) void greedy_edge_kernel(
    const double *S_all, const double *D_all, int n, int depot, int32_t *tour_out, double *score_out, double *cost_out,
    int32_t *edges_out, int32_t *rounds_out, int32_t *status_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int b = blockIdx.x, tid = threadIdx.x, nthr = blockDim.x;
    const int lane = tid & (kLanes - 1), wave = tid / kLanes, nwaves = nthr / kLanes;

    unsigned char *p = smem;
    GreedyCtl *ctl = reinterpret_cast<GreedyCtl *>(p);  p += ge_r16(sizeof(GreedyCtl));
    uint64_t *candkey = reinterpret_cast<uint64_t *>(p);  p += ge_r16((size_t)n * 8);
    double *dbuf = reinterpret_cast<double *>(p);  p += ge_r16((size_t)n * 8);
    int32_t *deg = reinterpret_cast<int32_t *>(p);  p += ge_r16((size_t)n * 4);
    int32_t *nbr = reinterpret_cast<int32_t *>(p);  p += ge_r16((size_t)n * 8);
    int32_t *other = reinterpret_cast<int32_t *>(p);  p += ge_r16((size_t)n * 4);
    int32_t *candj = reinterpret_cast<int32_t *>(p);  p += ge_r16((size_t)n * 4);
    int32_t *list = reinterpret_cast<int32_t *>(p);  p += ge_r16((size_t)(n + 1) * 4);      // rows to rescan; at the end the tour
    uint32_t *elist = reinterpret_cast<uint32_t *>(p);                                        // accepted edges, i << 16 | j
    double *sbuf = reinterpret_cast<double *>(candkey);                                       // the tour's keys, after the rounds

    const double *S = S_all + (size_t)b * n * n;
    const double *D = D_all ? D_all + (size_t)b * n * n : nullptr;
    int32_t *tour = tour_out + (size_t)b * (n + 1);
    int32_t *edges = edges_out ? edges_out + (size_t)b * n * 2 : nullptr;

    // ---- every row once: the first candidates, and the refusal of an off-diagonal entry that is not finite -------------------------
    if (tid == 0) { ctl->bad = 0; ctl->nlist = 0; ctl->accepted = 0; ctl->e0 = 0; ctl->e1 = 0; }
    if (tid < n) { deg[tid] = 0; nbr[2 * tid] = tid; nbr[2 * tid + 1] = tid; other[tid] = tid; }
    __syncthreads();
    {
        bool bad = false;
        for (int u = wave; u < n; u += nwaves) {
            uint64_t bk;
            int bj;
            scan_row<true>(S + (size_t)u * n, n, u, u, deg, lane, bk, bj, bad);
            if (lane == 0) { candkey[u] = bk; candj[u] = bj; }
        }
        if (bad) ctl->bad = 1;
    }
    __syncthreads();
    int accepted = 0, rounds = 0;
    const bool refused = ctl->bad != 0;

    // ---- the rounds ------------------------------------------------------------------------------------------------------------
    while (!refused && accepted < n - 1) {
        // 1. the end nodes whose cached candidate is no longer valid (in the first round: none)
        {
            bool stale = false;
            if (tid < n && deg[tid] < 2) {
                const int j = candj[tid];
                stale = j >= n || deg[j] >= 2 || j == other[tid];
            }
            const unsigned long long bm = __ballot(stale);
            if (bm != 0ull) {
                int base = 0;
                if (lane == 0) base = atomicAdd(&ctl->nlist, __popcll((long long)bm));
                base = __shfl(base, 0);
                if (stale) list[base + __popcll((long long)(bm & ((1ull << lane) - 1ull)))] = tid;
            }
        }
        __syncthreads();
        const int nl = ctl->nlist;
        for (int r = wave; r < nl; r += nwaves) {
            const int u = list[r];
            uint64_t bk;
            int bj;
            bool unused = false;
            scan_row<false>(S + (size_t)u * n, n, u, other[u], deg, lane, bk, bj, unused);
            if (lane == 0) { candkey[u] = bk; candj[u] = bj; }
        }
        __syncthreads();

        // 2. dominance, decided by the thread of the smaller end; reads only
        bool dom = false;
        int v = 0;
        if (tid < n && deg[tid] < 2) {
            const int u = tid;
            const int j = candj[u];
            if (j < n && u < j && candj[j] == u) {
                const uint64_t ek = candkey[u];
                const int a = other[u], c = other[j];
                dom = candkey[j] == ek;
                if (a != u) dom = dom && cand_above(candkey[a], a, candj[a], ek, u, j);
                if (c != j) dom = dom && cand_above(candkey[c], c, candj[c], ek, u, j);
                v = j;
            }
        }
        int slot = 0;
        {
            const unsigned long long bm = __ballot(dom);
            if (bm != 0ull) {
                int base = 0;
                if (lane == 0) base = atomicAdd(&ctl->accepted, __popcll((long long)bm));
                base = __shfl(base, 0);
                slot = base + __popcll((long long)(bm & ((1ull << lane) - 1ull)));
            }
        }
        if (tid == 0) ctl->nlist = 0;
        __syncthreads();
        const int acc = ctl->accepted;
        ++rounds;
        if (acc == accepted) break;                       // never with a symmetric S: the smallest valid edge is dominant
        accepted = acc;

        // 3. accept: the fragments of two dominant edges are disjoint, so every word below has one writer
        if (dom) {
            const int u = tid, a = other[u], c = other[v];
            nbr[2 * u + deg[u]] = v;
            nbr[2 * v + deg[v]] = u;
            deg[u] += 1;
            deg[v] += 1;
            other[a] = c;
            other[c] = a;
            if (slot < n) elist[slot] = ((uint32_t)u << 16) | (uint32_t)v;      // always: at most n - 1 edges join n nodes
        }
        __syncthreads();
    }

    if (refused || accepted < n - 1) {
        for (int q = tid; q <= n; q += nthr) tour[q] = -1;
        if (edges)
            for (int q = tid; q < 2 * n; q += nthr) edges[q] = -1;
        if (tid == 0) {
            score_out[b] = NAN;
            cost_out[b] = NAN;
            rounds_out[b] = rounds;
            status_out[b] = refused ? kGreedyEdgeStatusBadScore : kGreedyEdgeStatusStalled;
        }
        return;
    }

    // ---- the closing edge: the two nodes of degree 1 are each other's far end ----------------------------------------------------
    if (tid < n && deg[tid] == 1) {
        const int o = other[tid];
        nbr[2 * tid + 1] = o;
        if (tid < o) { ctl->e0 = tid; ctl->e1 = o; }
    }
    __syncthreads();

    // ---- the edges in acceptance order = ascending (key, i, j): ranked by counting -------------------------------------------------
    if (edges) {
        uint64_t *ekey = candkey;
        uint64_t ki = 0ull;
        uint32_t ei = 0u;
        if (tid < n - 1) {
            ei = elist[tid];
            ki = ord_key(S[(size_t)(ei >> 16) * n + (ei & 0xFFFFu)]);
            ekey[tid] = ki;
        }
        __syncthreads();
        if (tid < n - 1) {
            int rank = 0;
            for (int m = 0; m < n - 1; ++m) {
                const uint64_t km = ekey[m];
                const uint32_t em = elist[m];
                rank += (km < ki || (km == ki && em < ei)) ? 1 : 0;
            }
            edges[2 * rank] = (int32_t)(ei >> 16);
            edges[2 * rank + 1] = (int32_t)(ei & 0xFFFFu);
        }
        if (tid == 0) { edges[2 * (n - 1)] = ctl->e0; edges[2 * (n - 1) + 1] = ctl->e1; }
        __syncthreads();
    }

    // ---- the tour from the depot, towards its smaller neighbour -------------------------------------------------------------------
    if (tid == 0) {
        const int a = nbr[2 * depot], c = nbr[2 * depot + 1];
        int prev = depot, cur = a < c ? a : c;
        list[0] = depot;
        for (int q = 1; q < n; ++q) {
            list[q] = cur;
            const int x = nbr[2 * cur], y = nbr[2 * cur + 1];
            const int nxt = x == prev ? y : x;
            prev = cur;
            cur = nxt;
        }
        list[n] = depot;
    }
    __syncthreads();
    for (int q = tid; q <= n; q += nthr) tour[q] = list[q];
    if (tid < n) {
        const int x = list[tid], y = list[tid + 1];
        const int lo = x < y ? x : y, hi = x < y ? y : x;
        sbuf[tid] = S[(size_t)lo * n + hi];
        dbuf[tid] = D ? D[(size_t)x * n + y] : 0.0;
    }
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        for (int q = 0; q < n; ++q) s = s + sbuf[q];
        score_out[b] = s;
        rounds_out[b] = rounds;
        status_out[b] = 0;
    }
    if (tid == nthr - 1) {
        double c = NAN;
        if (D) {
            c = 0.0;
            for (int q = 0; q < n; ++q) c = c + dbuf[q];
        }
        cost_out[b] = c;
    }
}

}  // namespace

int greedy_edge_waves(int n) {
    const int w = (n + 15) / 16;
    return w < 1 ? 1 : (w > kGreedyEdgeMaxWaves ? kGreedyEdgeMaxWaves : w);
}

size_t greedy_edge_lds_bytes(int n) {
    return ge_r16(sizeof(GreedyCtl)) + 2 * ge_r16((size_t)n * 8) + ge_r16((size_t)n * 4) + ge_r16((size_t)n * 8) + 2 * ge_r16((size_t)n * 4) +
           ge_r16((size_t)(n + 1) * 4) + ge_r16((size_t)n * 4);
}

hipError_t launch_greedy_edge(const double *S, const double *D, int B, int n, int depot, int32_t *tour, double *score, double *cost,
                              int32_t *edges, int32_t *rounds, int32_t *status, hipStream_t stream) {
    if (B == 0) return hipSuccess;
    (void)hipGetLastError();
    hipLaunchKernelGGL(greedy_edge_kernel, dim3((unsigned)B), dim3(kLanes * greedy_edge_waves(n)), greedy_edge_lds_bytes(n), stream, S, D, n,
                       depot, tour, score, cost, edges, rounds, status);
    return hipGetLastError();
}

}  // namespace gnngls
