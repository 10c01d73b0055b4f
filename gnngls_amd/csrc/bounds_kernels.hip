// bounds_kernels.hip -- the Held-Karp 1-tree lower bound on MI355X (gfx950), hand-written HIP.
//
// Stands in for the denominator of the reference's gap, Concorde's optimum stored in its instance files (scripts/test.py:62,104,
// gnngls/__init__.py:55-60), with the one certified quantity this project can compute: max_k w(pi_k) <= optimum, the subgradient
// ascent over minimum 1-trees of oracle/one_tree.c (one_tree_lower_bound, min_one_tree).  Every fp64 operation of that file is
// repeated here in its order (the unit is compiled with contraction off), so the bound has the oracle's bits.
//
// One workgroup per instance, the whole ascent in one launch, no host round trip.  Node v lives on thread v % T, slot v / T
// (T = workgroup size): its Prim key, parent, in-tree flag, degree, potential and best potential are registers for the whole
// ascent.  Up to n = 256 the workgroup is ONE wavefront with one to four nodes per lane: the arg-min of a Prim step is a DPP
// reduction and the Prim loop holds no barrier.  Above, two to four wavefronts of four nodes per lane and the workgroup arg-min
// of the search kernel (one barrier per step).  The only LDS state is a copy of pi (the step reads pi[u] of the node just added,
// which lives in another lane) and the exchange slots of the reductions.  Row u of the matrix is read from global memory, one
// coalesced row per Prim step; the symmetry pass in front of the ascent has pulled the instance into L2.
//
// [exact] Prim (one_tree.c:27-38): `u` = first strictly smallest key among the outside nodes 1..n-1 = lexicographic min of
// (key, v); the reduction carries v's parent in the low bits of the key word (distinct v: the order is v's).  Every value that
// steers the ascent -- u, total, w, best, the stall counter, the step factor -- is computed by every lane from uniform inputs.
// [exact] total += key[u] in Prim order, then m1 + m2 (one_tree.c:31,44); the reductions return (+)0.0 for a key of -0.0, which
// no sum can tell apart: total starts at +0.0 and a sum of fp64 values is -0.0 only if every term is.
#include <hip/hip_runtime.h>
#include <float.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "bounds_kernels.h"
#include "gls_policy.h"

#pragma clang fp contract(off)

namespace gnngls {

#include "gls_common.h"

namespace {

constexpr int kBoundSlots = 4;         // nodes per lane at most
constexpr int kBoundWaves = 4;         // wavefronts per instance at most

__host__ __device__ inline size_t bound_r16(size_t x) { return (x + 15) & ~size_t(15); }
__host__ __device__ inline size_t bound_lds_bytes(int n) {
    return bound_r16(sizeof(Ctl)) + 2 * kBoundWaves * sizeof(int) + (size_t)n * sizeof(double);
}

__device__ __forceinline__ int wave_sum(int x) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m);
    return x;
}

template <int SLOTS, bool MULTI>
__global__ __launch_bounds__(MULTI ? 64 * kBoundWaves : 64) void one_tree_kernel(const double *D, const double *ubs, int n, int max_iters,
                                                                                 double *bound, double *pi_out, int32_t *iters,
                                                                                 int32_t *exit_kind, int32_t *status) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    Ctl *ctl = reinterpret_cast<Ctl *>(smem);
    int *red = reinterpret_cast<int *>(smem + bound_r16(sizeof(Ctl)));                                   // [2][kBoundWaves]
    double *pi_s = reinterpret_cast<double *>(smem + bound_r16(sizeof(Ctl)) + 2 * kBoundWaves * sizeof(int));   // [n]
    const int b = blockIdx.x, tid = threadIdx.x, nthr = MULTI ? (int)blockDim.x : kWave;
    const int lane = tid & (kWave - 1), wave = tid / kWave, nwaves = MULTI ? nthr / kWave : 1;
    const double *c = D + (size_t)b * n * n;

    // the bound is a bound for symmetric costs only: one pass over the upper triangle against the lower one, bit by bit
    int bad = 0;
    for (int i = 0; i < n - 1; ++i)
        for (int j = i + 1 + tid; j < n; j += nthr)
            bad |= __double_as_longlong(c[(size_t)i * n + j]) != __double_as_longlong(c[(size_t)j * n + i]);
    if (__syncthreads_or(bad)) {
        if (tid == 0) { status[b] = GNNGLS_STATUS_ASYMMETRIC_DEV; bound[b] = NAN; }
        return;
    }
    if (tid == 0) status[b] = 0;

    double key[SLOTS], pi[SLOTS], bpi[SLOTS], c0[SLOTS];
    int par[SLOTS], deg[SLOTS];
    bool valid[SLOTS];                 // a node of Prim's set: 1..n-1
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) {
        const int v = tid + s * nthr;
        pi[s] = 0.0; bpi[s] = 0.0;
        valid[s] = v >= 1 && v < n;
        c0[s] = valid[s] ? c[v] : 0.0;
    }
    const double ub = ubs[b];
    double best = -DBL_MAX, lambda = 2.0;                // one_tree.c:56-58
    int stall = 0, built = 0, kind = BOUND_EXIT_ITERS, phase = 0, rphase = 0;
    const int period = n < 50 ? 25 : n / 2;
    int it = 0;
    for (; it < max_iters && lambda > 1e-5; ++it) {
#pragma unroll
        for (int s = 0; s < SLOTS; ++s) {
            const int v = tid + s * nthr;
            if (v < n) pi_s[v] = pi[s];
        }
        __syncthreads();
        double sum_pi = 0.0;                             // one_tree.c:60-61: in node order
        {
            int i = 0;
            for (; i + 4 <= n; i += 4) {
                const double p0 = pi_s[i], p1 = pi_s[i + 1], p2 = pi_s[i + 2], p3 = pi_s[i + 3];
                sum_pi += p0; sum_pi += p1; sum_pi += p2; sum_pi += p3;
            }
            for (; i < n; ++i) sum_pi += pi_s[i];
        }

        // ---- min_one_tree (one_tree.c:23-46) ----
        unsigned in = 0;
#pragma unroll
        for (int s = 0; s < SLOTS; ++s) { key[s] = DBL_MAX; par[s] = -1; deg[s] = 0; }
        double total = 0.0;
        int u = 1, p = -1;                               // key[1] = 0 against DBL_MAX: the first node is node 1, without a parent
        for (int step = 1; step < n; ++step) {
            if (step > 1) {
                double bd = INFINITY;
                int bk = kNoKey;
#pragma unroll
                for (int s = 0; s < SLOTS; ++s) {
                    const int k = ((tid + s * nthr) << 10) | (par[s] & 1023);
                    if (valid[s] && !((in >> s) & 1u) && (bk == kNoKey || better<false>(key[s], k, bd, bk))) { bd = key[s]; bk = k; }
                }
                block_reduce_best<false>(ctl, phase, wave, nwaves, lane, bd, bk);
                u = bk >> 10; p = bk & 1023;
                if ((unsigned)(u - 1) >= (unsigned)(n - 1)) { u = 1; p = 1; }    // non-finite costs only: unspecified, but in range
                total += bd;                                                     // one_tree.c:31
            }
#pragma unroll
            for (int s = 0; s < SLOTS; ++s) {
                const int v = tid + s * nthr;
                if (v == u) { in |= 1u << s; if (step > 1) deg[s]++; }
                if (v == p) deg[s]++;
            }
            if (step == n - 1) break;                    // nothing left outside
            const double *cu = c + (size_t)u * n;
            const double piu = pi_s[u];
            double row[SLOTS];
#pragma unroll
            for (int s = 0; s < SLOTS; ++s) row[s] = (valid[s] && !((in >> s) & 1u)) ? cu[tid + s * nthr] : 0.0;
#pragma unroll
            for (int s = 0; s < SLOTS; ++s) {
                if (!valid[s] || ((in >> s) & 1u)) continue;
                const double w = (row[s] + piu) + pi[s];                         // one_tree.c:35
                if (w < key[s]) { key[s] = w; par[s] = u; }
            }
        }
        // the two cheapest edges at node 0 (one_tree.c:39-44): the two lexicographically smallest (weight, node)
        const double pi0 = pi_s[0];
        double w0[SLOTS];
#pragma unroll
        for (int s = 0; s < SLOTS; ++s) w0[s] = (c0[s] + pi0) + pi[s];
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
        total += m1 + m2;
        int sq = 0;
#pragma unroll
        for (int s = 0; s < SLOTS; ++s) {
            const int v = tid + s * nthr;
            if (v == 0) deg[s] = 2;
            if (v == a1) deg[s]++;
            if (v == a2) deg[s]++;
            if (v < n) sq += (deg[s] - 2) * (deg[s] - 2);
        }
        ++built;

        // ---- the ascent step (one_tree.c:62-70) ----
        const double w = total - 2.0 * sum_pi;
        if (w > best) {
            best = w; stall = 0;
#pragma unroll
            for (int s = 0; s < SLOTS; ++s) bpi[s] = pi[s];
        } else {
            stall++;
        }
        int norm = wave_sum(sq);                         // <= (2n)^2 = 2^22
        if (MULTI) {
            if (lane == 0) red[rphase * kBoundWaves + wave] = norm;
            __syncthreads();
            norm = 0;
            for (int k = 0; k < nwaves; ++k) norm += red[rphase * kBoundWaves + k];
            rphase ^= 1;
        }
        if (norm == 0) { kind = BOUND_EXIT_TOUR; break; }
        if (stall >= period) {
            lambda *= 0.5; stall = 0;
#pragma unroll
            for (int s = 0; s < SLOTS; ++s) pi[s] = bpi[s];
            continue;
        }
        const double gap = ub > w ? ub - w : 1e-3 * (ub > 0 ? ub : 1.0);
        const double step = lambda * gap / (double)norm;
#pragma unroll
        for (int s = 0; s < SLOTS; ++s)
            if (tid + s * nthr < n) pi[s] += step * (double)(deg[s] - 2);
    }
    if (kind != BOUND_EXIT_TOUR) kind = it >= max_iters ? BOUND_EXIT_ITERS : BOUND_EXIT_STEP;
    if (tid == 0) { bound[b] = best; iters[b] = built; exit_kind[b] = kind; }
    if (pi_out) {
#pragma unroll
        for (int s = 0; s < SLOTS; ++s) {
            const int v = tid + s * nthr;
            if (v < n) pi_out[(size_t)b * n + v] = bpi[s];
        }
    }
}

template <int SLOTS, bool MULTI>
hipError_t launch(const double *D, const double *ub, int B, int n, int max_iters, double *bound, double *pi, int32_t *iters,
                  int32_t *exit_kind, int32_t *status, int threads, hipStream_t stream) {
    (void)hipGetLastError();
    hipLaunchKernelGGL((one_tree_kernel<SLOTS, MULTI>), dim3(B), dim3(threads), bound_lds_bytes(n), stream, D, ub, n, max_iters, bound,
                       pi, iters, exit_kind, status);
    return hipGetLastError();
}

}  // namespace

int one_tree_threads(int n) { return n <= kWave * kBoundSlots ? kWave : kWave * ((n + kWave * kBoundSlots - 1) / (kWave * kBoundSlots)); }

int one_tree_lds_bytes(int n) { return (int)bound_lds_bytes(n); }

hipError_t launch_one_tree_bound(const double *D, const double *ub, int B, int n, int max_iters, double *bound, double *pi,
                                 int32_t *iters, int32_t *exit_kind, int32_t *status, hipStream_t stream) {
    static_assert(kOneTreeMaxN == kWave * kBoundSlots * kBoundWaves && kOneTreeMaxN <= 1024, "node and parent share a 20-bit key");
    const int threads = one_tree_threads(n);
#define GNNGLS_BOUND_ARGS D, ub, B, n, max_iters, bound, pi, iters, exit_kind, status, threads, stream
    if (n <= kWave) return launch<1, false>(GNNGLS_BOUND_ARGS);
    if (n <= 2 * kWave) return launch<2, false>(GNNGLS_BOUND_ARGS);
    if (n <= 3 * kWave) return launch<3, false>(GNNGLS_BOUND_ARGS);
    if (n <= 4 * kWave) return launch<4, false>(GNNGLS_BOUND_ARGS);
    return launch<4, true>(GNNGLS_BOUND_ARGS);
#undef GNNGLS_BOUND_ARGS
}

}  // namespace gnngls
