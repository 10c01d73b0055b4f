// aco_kernels.hip -- a MAX-MIN ant system (Stuetzle & Hoos) over any edge heuristic on MI355X (gfx950), hand-written HIP.
//
// The reference has no counterpart: it uses an edge score only as the utility of guided local search.  include/gnngls_hip.h
// states the definition (gnngls_aco_run), gnngls_amd.host.aco restates it in NumPy and the device matches it bit for bit.
//
// One workgroup per instance runs all K iterations of a launch; it has min(R, 16) wavefronts and ant a walks on wavefront
// a % W, in rounds.  A walk is the sampled walk of sampling_kernels.hip on w_j = tau[i,j] * H[i,j]: node j on lane j % 64, slot
// j / 64, visited bits, weights and the tour in registers, two coalesced row reads per step.  The scan, running-sum and pick
// code below is carried over from that unit (tests/test_aco_gpu.py pins the two copies to each other).  A finished walk
// gathers its edge lengths (one per lane and slot), sums them in tour order from node 0 by reading lane after lane, and a
// wavefront keeps the cheapest of its ants' tours, rotated to start at node 0, in LDS.  After a barrier every thread reduces
// the W candidates to the iteration's winner, so everything that steers a barrier -- the early end, the winner, the best
// cost, the schedule of the deposit tour -- is workgroup-uniform.  The deposit tour is published as succ[] / pred[] in LDS and
// all threads sweep the n * n entries of tau in global memory, a row per wavefront, coalesced.  tau is written and re-read by
// this workgroup only: plain stores, then the workgroup's barrier, as guided_or_opt_kernel treats its penalty counters.
//
// [exact] every fp64 operation is one add, multiply or divide rounded once (contraction off); the clamp is two compares and
// selects, so a NaN stays a NaN.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "aco_kernels.h"
#include "philox.h"

#pragma clang fp contract(off)

namespace gnngls {

namespace {

constexpr int kLanes = 64;

struct AcoCtl {
    double wcost[kAcoMaxWaves];          // per wavefront: the cost of its cheapest ant
    int32_t want[kAcoMaxWaves];          // ... that ant's index (-1: none finished)
    int32_t wbad[kAcoMaxWaves];          // ... whether one of its ants met refused weights or a cost that is not finite
};

__host__ __device__ inline size_t aco_r16(size_t x) { return (x + 15) & ~(size_t)15; }

// ---- carried over from sampling_kernels.hip ----------------------------------------------------------------------------------
// inclusive doubling scan over the 64 lanes: round d adds the value lane l - d held before the round
__device__ __forceinline__ double lane_scan(double v, int lane) {
#pragma unroll
    for (int d = 1; d < kLanes; d <<= 1) {
        const double t = __shfl_up(v, d);
        if (lane >= d) v = v + t;
    }
    return v;
}

// run[s] = base_s + scan of slot s; returns the total (sampling_kernels.h: summation order)
template <int SLOTS>
__device__ __forceinline__ double running_sums(const double (&p)[SLOTS], int nslots, int lane, double (&run)[SLOTS]) {
    double base = 0.0;
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) {
        run[s] = 0.0;
        if (s < nslots) {
            const double c = lane_scan(p[s], lane);
            run[s] = base + c;
            base = base + __shfl(c, kLanes - 1);
        }
    }
    return base;
}

// the walk of sampling_kernels.h from `start` with invert = 0 on w_j = tau[i,j] * H[i,j]; -> true where a step met refused weights
template <int SLOTS>
__device__ __forceinline__ bool walk(const double *tau, const double *H, int n, int nslots, int lane, int start, uint64_t seed,
                                     uint32_t c0, uint32_t c1, const double *uw, int32_t (&t)[SLOTS + 1]) {
    unsigned closed = 0;                   // bit s: node lane + 64 s is no candidate (visited, or >= n)
#pragma unroll
    for (int s = 0; s < SLOTS; ++s)
        if (lane + kLanes * s >= n) closed |= 1u << s;
    if (lane == (start & (kLanes - 1))) closed |= 1u << (start / kLanes);
#pragma unroll
    for (int s = 0; s <= SLOTS; ++s) t[s] = start;        // positions 0 and n; the others are overwritten

    int cur = start;
    for (int k = 1; k < n; ++k) {
        const double *trow = tau + (size_t)cur * n, *hrow = H + (size_t)cur * n;
        double p[SLOTS], run[SLOTS];
        bool cand[SLOTS];
        bool inf = false, signed_or_nan = false, positive = false;
#pragma unroll
        for (int s = 0; s < SLOTS; ++s) {
            const int j = lane + kLanes * s;
            cand[s] = !((closed >> s) & 1u);
            p[s] = cand[s] ? trow[j] * hrow[j] : 0.0;     // cand implies j < n
            inf |= cand[s] && isinf(p[s]);
        }
        if (__ballot(inf) != 0ull) {
#pragma unroll
            for (int s = 0; s < SLOTS; ++s) p[s] = (cand[s] && isinf(p[s])) ? 1.0 : 0.0;
        }
#pragma unroll
        for (int s = 0; s < SLOTS; ++s) {
            signed_or_nan |= cand[s] && !(p[s] >= 0.0);
            positive |= cand[s] && p[s] > 0.0;
        }
        bool zero_sum;
        if (__ballot(signed_or_nan) == 0ull) zero_sum = __ballot(positive) == 0ull;
        else zero_sum = running_sums<SLOTS>(p, nslots, lane, run) == 0.0;
        if (zero_sum) {
#pragma unroll
            for (int s = 0; s < SLOTS; ++s) p[s] = cand[s] ? 1.0 : 0.0;
        }
        bool refuse = false;
#pragma unroll
        for (int s = 0; s < SLOTS; ++s) refuse |= cand[s] && (!(p[s] >= 0.0) || isinf(p[s]));
        const double total = running_sums<SLOTS>(p, nslots, lane, run);
        if (__ballot(refuse) != 0ull || !(total > 0.0) || isinf(total)) return true;

        const double uu = uw ? uw[k - 1] : philox_uniform53(seed, c0, c1, (uint32_t)(k - 1), 2u);
        const double x = uu * total;
        int pick = -1, last = -1;
#pragma unroll
        for (int s = 0; s < SLOTS; ++s) {
            const bool live = cand[s] && p[s] > 0.0;
            const unsigned long long over = __ballot(live && run[s] > x), any = __ballot(live);
            if (pick < 0 && over != 0ull) pick = kLanes * s + (__ffsll((long long)over) - 1);
            if (any != 0ull) last = kLanes * s + (kLanes - 1 - __clzll((long long)any));
        }
        if (pick < 0) pick = last;                        // total > 0: some candidate has p > 0, so last >= 0
        pick = __builtin_amdgcn_readfirstlane(pick);

        if (lane == (pick & (kLanes - 1))) closed |= 1u << (pick / kLanes);
#pragma unroll
        for (int s = 0; s <= SLOTS; ++s)
            if (s == k / kLanes && lane == (k & (kLanes - 1))) t[s] = pick;
        cur = pick;
    }
    return false;
}
// ---- end of the carried-over code --------------------------------------------------------------------------------------------

// the value lane l (wave-uniform) holds
__device__ __forceinline__ double read_lane(double v, int l) {
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), l), lo = __builtin_amdgcn_readlane(__double2loint(v), l);
    return __hiloint2double(hi, lo);
}

template <int SLOTS>
__global__ __launch_bounds__(kLanes *kAcoMaxWaves) void aco_kernel(
    const double *D, const double *H, double *tau_io, int32_t *best_tour, double *best_cost_io, int n, int R, int K, long long iter0,
    double rho, double min_ratio, int gb_every, int spread_starts, uint64_t seed, const double *u, int32_t *iters_done, int32_t *status_out,
    double *trace_cost, int32_t *ant_tours, double *ant_cost) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int b = blockIdx.x, tid = threadIdx.x, nthr = blockDim.x;
    const int lane = tid & (kLanes - 1), wave = tid / kLanes, W = nthr / kLanes;
    const int nslots = (n + kLanes - 1) / kLanes;
    const size_t tlen = (size_t)n + 1;
    AcoCtl *ctl = reinterpret_cast<AcoCtl *>(smem);
    int32_t *best = reinterpret_cast<int32_t *>(smem + aco_r16(sizeof(AcoCtl)));
    int32_t *succ = best + aco_r16(tlen * sizeof(int32_t)) / sizeof(int32_t);
    int32_t *pred = succ + aco_r16((size_t)n * sizeof(int32_t)) / sizeof(int32_t);
    int32_t *wtours = pred + aco_r16((size_t)n * sizeof(int32_t)) / sizeof(int32_t);
    int32_t *wtour = wtours + (size_t)wave * tlen;       // this wavefront's cheapest tour of the iteration, from node 0

    const double *c = D + (size_t)b * n * n, *h = H + (size_t)b * n * n;
    double *tau = tau_io + (size_t)b * n * n;
    int32_t *bt = best_tour + (size_t)b * tlen;
    double *trace = trace_cost ? trace_cost + (size_t)b * K : nullptr;
    int32_t *atours = ant_tours ? ant_tours + (size_t)b * R * tlen : nullptr;
    double *acost = ant_cost ? ant_cost + (size_t)b * R : nullptr;

    for (int q = tid; q <= n; q += nthr) best[q] = bt[q];
    double best_cost = best_cost_io[b];
    const double keep = 1.0 - rho;
    int status = 0, done = 0;
    __syncthreads();

    for (int it = 0; it < K; ++it) {
        const unsigned long long g = (unsigned long long)iter0 + (unsigned long long)it;
        // ---- 1, 2: the walks and their costs; no barrier inside -----------------------------------------------------------
        double wc = 0.0;
        int wa = -1, wbad = 0;
        for (int a = wave; a < R; a += W) {
            const int start = spread_starts ? (int)((g + (unsigned long long)a) % (unsigned long long)n) : 0;
            const double *uw = u ? u + ((((size_t)b * K + it) * R + a) * (size_t)(n - 1)) : nullptr;
            int32_t t[SLOTS + 1];
            const bool bad = walk<SLOTS>(tau, h, n, nslots, lane, start, seed, (uint32_t)b, (uint32_t)(g * (unsigned long long)R + a), uw, t);
            double cost = NAN;
            int z = 0;
            if (!bad) {
                double e[SLOTS];                          // the length of the tour edge at walk position k = lane + 64 s
#pragma unroll
                for (int s = 0; s < SLOTS; ++s) {
                    const int k = lane + kLanes * s;
                    int nxt = __shfl_down(t[s], 1);
                    const int nx0 = __shfl(t[s + 1], 0);
                    if (lane == kLanes - 1) nxt = nx0;
                    e[s] = k < n ? c[(size_t)t[s] * n + nxt] : 0.0;
                    const unsigned long long at0 = __ballot(k < n && t[s] == 0);
                    if (at0 != 0ull) z = kLanes * s + (__ffsll((long long)at0) - 1);
                }
                z = __builtin_amdgcn_readfirstlane(z);
                cost = 0.0;                               // tour_cost of the tour rotated to node 0: positions z .. n-1, then 0 .. z-1
#pragma unroll
                for (int pass = 0; pass < 2; ++pass) {
                    const int lo = pass == 0 ? z : 0, hi = pass == 0 ? n : z;
#pragma unroll
                    for (int s = 0; s < SLOTS; ++s) {
                        const int from = lo - kLanes * s > 0 ? lo - kLanes * s : 0;
                        const int to = hi - kLanes * s < kLanes ? hi - kLanes * s : kLanes;
                        for (int l = from; l < to; ++l) cost = cost + read_lane(e[s], l);
                    }
                }
            }
            if (atours) {
                int32_t *out = atours + (size_t)a * tlen;
#pragma unroll
                for (int s = 0; s <= SLOTS; ++s) {
                    const int k = lane + kLanes * s;
                    if (bad) { if (k <= n) out[k] = -1; }
                    else if (k < n) out[k >= z ? k - z : k - z + n] = t[s];
                }
                if (!bad && lane == 0) out[n] = 0;
            }
            if (acost && lane == 0) acost[a] = cost;
            wbad |= bad || !isfinite(cost);
            if (!bad && (wa < 0 || cost < wc)) {          // ascending a: the lowest index among equal costs stays
                wc = cost;
                wa = a;
#pragma unroll
                for (int s = 0; s < SLOTS; ++s) {
                    const int k = lane + kLanes * s;
                    if (k < n) wtour[k >= z ? k - z : k - z + n] = t[s];
                }
                if (lane == 0) wtour[n] = 0;
            }
        }
        if (lane == 0) { ctl->wcost[wave] = wc; ctl->want[wave] = wa; ctl->wbad[wave] = wbad; }
        __syncthreads();
        // ---- 3, 4: early end and selection, by every thread from the same cells ---------------------------------------------
        int bad = 0, ib = -1, iw = 0;
        double mc = 0.0;
        for (int w = 0; w < W; ++w) {
            bad |= ctl->wbad[w];
            const int wa2 = ctl->want[w];
            const double wc2 = ctl->wcost[w];
            if (wa2 >= 0 && (ib < 0 || wc2 < mc || (wc2 == mc && wa2 < ib))) { mc = wc2; ib = wa2; iw = w; }
        }
        if (bad || ib < 0 || !(mc > 0.0)) { status = kAcoStatusBadWeights; break; }
        const int32_t *won = wtours + (size_t)iw * tlen;
        if (tid == 0 && trace) trace[it] = mc;
        if (mc < best_cost) {
            for (int q = tid; q <= n; q += nthr) best[q] = won[q];
            best_cost = mc;
        }
        __syncthreads();
        // ---- 5: evaporate, deposit, clamp --------------------------------------------------------------------------------
        const bool gb = gb_every > 0 && (g + 1ull) % (unsigned long long)gb_every == 0ull;
        const int32_t *X = gb ? best : won;
        for (int p = tid; p < n; p += nthr) {
            const int x = X[p], y = X[p + 1];
            if ((unsigned)x < (unsigned)n && (unsigned)y < (unsigned)n) { succ[x] = y; pred[y] = x; }
        }
        __syncthreads();
        const double dq = 1.0 / (gb ? best_cost : mc);
        const double rb = rho * best_cost;
        const double tau_max = 1.0 / rb;
        const double tau_min = tau_max * min_ratio;
        for (int i = wave; i < n; i += W) {
            const int si = succ[i], pi = pred[i];
            double *row = tau + (size_t)i * n;
            for (int j = lane; j < n; j += kLanes) {
                if (j == i) continue;
                double v = row[j] * keep;
                if (si == j || pi == j) v = v + dq;
                if (v < tau_min) v = tau_min;
                if (v > tau_max) v = tau_max;
                row[j] = v;
            }
        }
        done = it + 1;
        __syncthreads();                                  // tau is visible to the workgroup's next walks; succ / pred / wtours are free
    }
    __syncthreads();
    for (int q = tid; q <= n; q += nthr) bt[q] = best[q];
    if (tid == 0) { best_cost_io[b] = best_cost; iters_done[b] = done; status_out[b] = status; }
}

template <int SLOTS>
hipError_t launch(const double *D, const double *H, double *tau, int32_t *best_tour, double *best_cost, int B, int n, int R, int K,
                  long long iter0, double rho, double min_ratio, int gb_every, int spread_starts, uint64_t seed, const double *u,
                  int32_t *iters_done, int32_t *status, double *trace_cost, int32_t *ant_tours, double *ant_cost, hipStream_t stream) {
    const size_t lds = aco_lds_bytes(n, R);
    const int W = R < kAcoMaxWaves ? R : kAcoMaxWaves;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(aco_kernel<SLOTS>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    (void)hipGetLastError();
    hipLaunchKernelGGL(aco_kernel<SLOTS>, dim3((unsigned)B), dim3(kLanes * W), lds, stream, D, H, tau, best_tour, best_cost, n, R, K, iter0,
                       rho, min_ratio, gb_every, spread_starts, seed, u, iters_done, status, trace_cost, ant_tours, ant_cost);
    return hipGetLastError();
}

}  // namespace

size_t aco_lds_bytes(int n, int R) {
    const int W = R < kAcoMaxWaves ? R : kAcoMaxWaves;
    const size_t tlen = (size_t)n + 1;
    return aco_r16(sizeof(AcoCtl)) + aco_r16(tlen * sizeof(int32_t)) + 2 * aco_r16((size_t)n * sizeof(int32_t)) +
           aco_r16((size_t)W * tlen * sizeof(int32_t));
}

hipError_t launch_aco(const double *D, const double *H, double *tau, int32_t *best_tour, double *best_cost, int B, int n, int R, int K,
                      long long iter0, double rho, double min_ratio, int gb_every, int spread_starts, uint64_t seed, const double *u,
                      int32_t *iters_done, int32_t *status, double *trace_cost, int32_t *ant_tours, double *ant_cost,
                      hipStream_t stream) {
    if (B == 0) return hipSuccess;
    const int nslots = (n + kLanes - 1) / kLanes;        // instantiations: 1, 2, 4, 8, 16 nodes per lane
#define GNNGLS_ACO_LAUNCH(S) \
    launch<S>(D, H, tau, best_tour, best_cost, B, n, R, K, iter0, rho, min_ratio, gb_every, spread_starts, seed, u, iters_done, status, \
              trace_cost, ant_tours, ant_cost, stream)
    if (nslots <= 1) return GNNGLS_ACO_LAUNCH(1);
    if (nslots <= 2) return GNNGLS_ACO_LAUNCH(2);
    if (nslots <= 4) return GNNGLS_ACO_LAUNCH(4);
    if (nslots <= 8) return GNNGLS_ACO_LAUNCH(8);
    return GNNGLS_ACO_LAUNCH(16);
#undef GNNGLS_ACO_LAUNCH
}

}  // namespace gnngls
