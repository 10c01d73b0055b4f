// alpha_kernels.hip -- Helsgaun's alpha-nearness on MI355X (gfx950), hand-written HIP: a model-free, regret-like search guide.
//
// alpha(e) = (minimum 1-tree forced through e) - (minimum 1-tree) under the potentials pi of the Held-Karp ascent
// (bounds_kernels.hip returns them).  The contract is in include/gnngls_hip.h: canonical weight
//      w(i,j) = ((D[i][j] + pi[min(i,j)]) + pi[max(i,j)]) + 0.0          (the unit is compiled with contraction off),
// beta(i,j) = the largest w on the path between i and j in a minimum spanning tree of nodes 1..n-1 (the minimax-path value: the
// same for every minimum spanning tree), alpha(i,j) = w(i,j) - beta(i,j); node 0 is the special node: alpha(0,j) = w(0,j) - the
// second smallest w(0,.), floored at +0.0.  Every beta is one of the w, picked by comparisons: the output is bit-determined by
// (D, pi) whatever Prim's tie-breaks are.
//
// One workgroup per instance, one launch per batch, the node-to-lane layout of one_tree_kernel: node v lives on thread v % T, slot
// v / T; one wavefront with one to four nodes per lane up to n = 256, two to four wavefronts of four nodes per lane above.  A
// node's key, parent and potential are registers, pi also sits in LDS (the step reads pi[u] of the node just added).
//
// beta is kept IN PLACE in the output matrix.  When node u enters the tree with parent p and key k, every lane that owns an
// in-tree node v sets beta(u,v) = v == p ? k : max(beta(p,v), k) and writes it as [u][v] (one coalesced row) and [v][u]: row p is
// then one coalesced read per step, next to the row of D the step reads anyway.  A last elementwise pass turns beta into alpha and
// fills row 0, column 0 and the diagonal.  The Prim loop is a serial chain of n - 1 arg-mins with O(n) work each: its cost is
// latency (the arg-min, one load and one store round trip per step), not bandwidth.  (An LDS triangle for beta would take the
// store round trip out of the step; it is not built: nothing measured says it pays)
//
// [visibility] Rows of beta written in one step are read in later steps by other lanes of the same workgroup.  The writer ends its
// step with __threadfence_block(): a workgroup-scope release, on gfx950 `s_waitcnt vmcnt(0)` -- its stores have reached the
// vector L1 of the CU, which is write-through and is the one L1 every wavefront of a workgroup loads through (workgroups are not
// split over CUs), so no cache has to be written back or invalidated at this scope.  The readers' loads come behind the barrier of
// the next step's arg-min (__syncthreads: workgroup-scope acquire) in the multi-wavefront form, and behind the wait itself in
// the one-wavefront form, whose memory instructions issue in order.  No location is rewritten before the last pass: [u][.] and
// [.][u] are first read after u has entered.
#include <hip/hip_runtime.h>
#include <float.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "alpha_kernels.h"
#include "gls_policy.h"

#pragma clang fp contract(off)

namespace gnngls {

#include "gls_common.h"

namespace {

constexpr int kAlphaSlots = 4;         // nodes per lane at most
constexpr int kAlphaWaves = 4;         // wavefronts per instance at most

__host__ __device__ inline size_t alpha_r16(size_t x) { return (x + 15) & ~size_t(15); }
__host__ __device__ inline size_t alpha_lds(int n) { return alpha_r16(sizeof(Ctl)) + (size_t)n * sizeof(double); }

// the canonical weight of the pair (u, v), u != v: the potential of the smaller node is added first, so w(u,v) == w(v,u) bit for
// bit; the trailing + 0.0 reads a weight of -0.0 as +0.0 (the arg-min's order-preserving key does the same)
__device__ __forceinline__ double canon(double d, int u, double piu, int v, double piv) {
    const double lo = v < u ? piv : piu, hi = v < u ? piu : piv;
    return ((d + lo) + hi) + 0.0;
}

template <int SLOTS, bool MULTI>
__global__ __launch_bounds__(MULTI ? 64 * kAlphaWaves : 64) void alpha_kernel(const double *D, const double *pis, int n, double *alpha,
                                                                              int32_t *status) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    Ctl *ctl = reinterpret_cast<Ctl *>(smem);
    double *pi_s = reinterpret_cast<double *>(smem + alpha_r16(sizeof(Ctl)));                            // [n]
    const int b = blockIdx.x, tid = threadIdx.x, nthr = MULTI ? (int)blockDim.x : kWave;
    const int lane = tid & (kWave - 1), wave = tid / kWave, nwaves = MULTI ? nthr / kWave : 1;
    const double *c = D + (size_t)b * n * n;
    double *out = alpha + (size_t)b * n * n;

    // alpha is defined for symmetric costs only: one pass over the upper triangle against the lower one, bit by bit
    int bad = 0;
    for (int i = 0; i < n - 1; ++i)
        for (int j = i + 1 + tid; j < n; j += nthr)
            bad |= __double_as_longlong(c[(size_t)i * n + j]) != __double_as_longlong(c[(size_t)j * n + i]);
    if (__syncthreads_or(bad)) {
        if (tid == 0) status[b] = kAlphaStatusAsymmetric;
        for (size_t q = tid; q < (size_t)n * n; q += nthr) out[q] = NAN;
        return;
    }
    if (tid == 0) status[b] = 0;

    for (int v = tid; v < n; v += nthr) pi_s[v] = pis ? pis[(size_t)b * n + v] : 0.0;
    __syncthreads();

    double key[SLOTS], pi[SLOTS];
    int par[SLOTS];
    bool valid[SLOTS];                 // a node of Prim's set: 1..n-1
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) {
        const int v = tid + s * nthr;
        valid[s] = v >= 1 && v < n;
        pi[s] = v < n ? pi_s[v] : 0.0;
        key[s] = DBL_MAX; par[s] = -1;
    }

    // ---- Prim over nodes 1..n-1 under the canonical weight, beta of every pair (u, in-tree v) as u enters ----
    unsigned in = 0;
    int phase = 0;
    int u = 1, p = 1;                                    // the first node is node 1, without a parent
    double k = 0.0;
    for (int step = 1; step < n; ++step) {
        if (step > 1) {
            double bd = INFINITY;
            int bk = kNoKey;
#pragma unroll
            for (int s = 0; s < SLOTS; ++s) {
                const int q = ((tid + s * nthr) << 10) | (par[s] & 1023);
                if (valid[s] && !((in >> s) & 1u) && (bk == kNoKey || better<false>(key[s], q, bd, bk))) { bd = key[s]; bk = q; }
            }
            block_reduce_best<false>(ctl, phase, wave, nwaves, lane, bd, bk);
            u = bk >> 10; p = bk & 1023; k = bd;
            if ((unsigned)(u - 1) >= (unsigned)(n - 1)) u = 1;      // non-finite costs only: unspecified values, but every
            if ((unsigned)(p - 1) >= (unsigned)(n - 1)) p = 1;      // index stays in 1..n-1
        }
        const double *cu = c + (size_t)u * n;
        const double *bp = out + (size_t)p * n;
        const double piu = pi_s[u];
        const bool last = step == n - 1;                 // nothing left outside: no keys to lower
        double row[SLOTS], beta[SLOTS];
#pragma unroll
        for (int s = 0; s < SLOTS; ++s) {
            const int v = tid + s * nthr;
            const bool tree = (in >> s) & 1u;
            beta[s] = (tree && v != p) ? bp[v] : 0.0;
            row[s] = (valid[s] && !tree && v != u && !last) ? cu[v] : 0.0;
        }
#pragma unroll
        for (int s = 0; s < SLOTS; ++s) {
            const int v = tid + s * nthr;
            if (!((in >> s) & 1u)) continue;             // (empty at step 1)
            const double bt = v == p ? k : (beta[s] > k ? beta[s] : k);
            out[(size_t)u * n + v] = bt;
            out[(size_t)v * n + u] = bt;
        }
#pragma unroll
        for (int s = 0; s < SLOTS; ++s) {
            const int v = tid + s * nthr;
            if (v == u) in |= 1u << s;
            if (!valid[s] || ((in >> s) & 1u) || last) continue;
            const double w = canon(row[s], u, piu, v, pi[s]);
            if (w < key[s]) { key[s] = w; par[s] = u; }
        }
        __threadfence_block();                           // [visibility]: this step's rows of beta, before a later step reads them
    }

    // ---- node 0: the second smallest w(0, j), counted with multiplicity ----
    const double pi0 = pi_s[0];
    double w0[SLOTS];
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) w0[s] = valid[s] ? canon(c[tid + s * nthr], 0, pi0, tid + s * nthr, pi[s]) : 0.0;
    double m1 = INFINITY, m2 = INFINITY;
    int a1 = kNoKey, a2 = kNoKey;
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) {
        const int v = tid + s * nthr;
        if (valid[s] && (a1 == kNoKey || better<false>(w0[s], v, m1, a1))) { m1 = w0[s]; a1 = v; }
    }
    block_reduce_best<false>(ctl, phase, wave, nwaves, lane, m1, a1);
    const int first = a1;
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) {
        const int v = tid + s * nthr;
        if (valid[s] && v != first && (a2 == kNoKey || better<false>(w0[s], v, m2, a2))) { m2 = w0[s]; a2 = v; }
    }
    block_reduce_best<false>(ctl, phase, wave, nwaves, lane, m2, a2);
    __syncthreads();                                     // every row of beta is written and visible (the fences above)

    // ---- beta -> alpha in place, row by row: element [i][j] is read and written by the lane of node j ----
    for (int i = 0; i < n; ++i) {
        const double *ci = c + (size_t)i * n;
        double *oi = out + (size_t)i * n;
        const double pii = pi_s[i];
        double d[SLOTS], beta[SLOTS];
#pragma unroll
        for (int s = 0; s < SLOTS; ++s) {
            const int j = tid + s * nthr;
            d[s] = (j < n && j != i) ? ci[j] : 0.0;
            beta[s] = (valid[s] && i > 0 && j != i) ? oi[j] : 0.0;
        }
#pragma unroll
        for (int s = 0; s < SLOTS; ++s) {
            const int j = tid + s * nthr;
            if (j >= n) continue;
            double a = 0.0;                              // the diagonal
            if (j != i) {
                const double w = canon(d[s], i, pii, j, pi[s]);
                if (i == 0 || j == 0) { const double t = w - m2; a = t > 0.0 ? t : 0.0; }
                else a = w - beta[s];
            }
            oi[j] = a;
        }
    }
}

template <int SLOTS, bool MULTI>
hipError_t launch(const double *D, const double *pi, int B, int n, double *alpha, int32_t *status, int threads, hipStream_t stream) {
    (void)hipGetLastError();
    hipLaunchKernelGGL((alpha_kernel<SLOTS, MULTI>), dim3(B), dim3(threads), alpha_lds(n), stream, D, pi, n, alpha, status);
    return hipGetLastError();
}

}  // namespace

int alpha_threads(int n) { return n <= kWave * kAlphaSlots ? kWave : kWave * ((n + kWave * kAlphaSlots - 1) / (kWave * kAlphaSlots)); }

int alpha_lds_bytes(int n) { return (int)alpha_lds(n); }

hipError_t launch_alpha_nearness(const double *D, const double *pi, int B, int n, double *alpha, int32_t *status, hipStream_t stream) {
    static_assert(kAlphaMaxN == kWave * kAlphaSlots * kAlphaWaves && kAlphaMaxN <= 1024, "node and parent share a 20-bit key");
    const int threads = alpha_threads(n);
#define GNNGLS_ALPHA_ARGS D, pi, B, n, alpha, status, threads, stream
    if (n <= kWave) return launch<1, false>(GNNGLS_ALPHA_ARGS);
    if (n <= 2 * kWave) return launch<2, false>(GNNGLS_ALPHA_ARGS);
    if (n <= 3 * kWave) return launch<3, false>(GNNGLS_ALPHA_ARGS);
    if (n <= 4 * kWave) return launch<4, false>(GNNGLS_ALPHA_ARGS);
    return launch<4, true>(GNNGLS_ALPHA_ARGS);
#undef GNNGLS_ALPHA_ARGS
}

}  // namespace gnngls
