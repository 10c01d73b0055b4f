// sampling_kernels.hip -- sampled nearest-neighbour walks on MI355X (gfx950), hand-written HIP.
//
// Replaces (reference file:line, gnngls/...):
//   algorithms.py:21-50   probabilistic_nearest_neighbour, with the uniforms of np.random.choice as an explicit input
//                         (sampling_kernels.h states the walk, its summation order and the generator)
//
// One wavefront runs one walk; the grid holds the B * R walks of a launch and no step leaves the device.  Node j lives on lane
// j % 64, slot j / 64: its visited bit and its candidate weight are registers, and so is the tour (position k on lane k % 64).
// A step reads row i of the instance's matrix from global memory, one coalesced 512 B segment per slot; the R walks of an
// instance share the matrix in L2.  The running sums are a doubling scan over the lanes per slot (6 cross-lane moves of an
// fp64 value) and a serial chain of slot totals; the pick is a ballot.  Everything that steers a walk -- the inf / all-zero /
// bad-weight decisions, total, x, the picked node -- is computed by every lane from wave-uniform values.
//
// [exact] the order of the fp64 adds is the one sampling_kernels.h states; the unit is compiled with contraction off, and a
// masked node adds +0.0 (x + 0.0 == x for every x the sums can hold, base_0 being +0.0).
// [exact] sum(p) == 0 (algorithms.py:39): when no candidate weight is negative or NaN the sum in ANY order is 0 iff every
// candidate is (+-)0, so the scan is only run for that test when a negative or NaN weight is present.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "philox.h"
#include "sampling_kernels.h"

#pragma clang fp contract(off)

namespace gnngls {

namespace {

constexpr int kLanes = 64;

// the walks' stream of philox.h: counter (b, r, step, 0)
__device__ __forceinline__ double uniform53(uint64_t seed, uint32_t b, uint32_t r, uint32_t s) {
    return philox_uniform53(seed, b, r, s, 0u);
}

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

template <int SLOTS>
__global__ __launch_bounds__(64) void sample_nn_kernel(const double *W, int n, int R, int depot, int invert, uint64_t seed,
                                                       const double *u, int32_t *tours, int32_t *status) {
    const int lane = threadIdx.x;
    const size_t walk = blockIdx.x;
    const int b = (int)(walk / (size_t)R), r = (int)(walk % (size_t)R);
    const double *Wb = W + (size_t)b * n * n;
    const double *uw = u ? u + walk * (size_t)(n - 1) : nullptr;
    const int nslots = (n + kLanes - 1) / kLanes;

    unsigned closed = 0;                   // bit s: node lane + 64 s is no candidate (visited, or >= n)
    int32_t t[SLOTS + 1];                  // tour position k on lane k % 64, slot k / 64 (k = 0 .. n)
#pragma unroll
    for (int s = 0; s < SLOTS; ++s)
        if (lane + kLanes * s >= n) closed |= 1u << s;
    if (lane == (depot & (kLanes - 1))) closed |= 1u << (depot / kLanes);
#pragma unroll
    for (int s = 0; s <= SLOTS; ++s) t[s] = depot;        // positions 0 and n; the others are overwritten

    int cur = depot;
    bool bad = false;
    for (int k = 1; k < n; ++k) {
        const double *row = Wb + (size_t)cur * n;
        double p[SLOTS], run[SLOTS];
        bool cand[SLOTS];
        bool inf = false, signed_or_nan = false, positive = false;
#pragma unroll
        for (int s = 0; s < SLOTS; ++s) {
            const int j = lane + kLanes * s;
            cand[s] = !((closed >> s) & 1u);
            p[s] = cand[s] ? row[j] : 0.0;                // cand implies j < n
            inf |= cand[s] && isinf(p[s]);
        }
        if (__ballot(inf) != 0ull) {                      // algorithms.py:34-36
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
        if (zero_sum) {                                   // algorithms.py:39-40
#pragma unroll
            for (int s = 0; s < SLOTS; ++s) p[s] = cand[s] ? 1.0 : 0.0;
        }
        if (invert) {                                     // algorithms.py:43-44
#pragma unroll
            for (int s = 0; s < SLOTS; ++s) p[s] = cand[s] ? 1.0 / p[s] : 0.0;
        }
        bool refuse = false;                              // what np.random.choice refuses (algorithms.py:46)
#pragma unroll
        for (int s = 0; s < SLOTS; ++s) refuse |= cand[s] && (!(p[s] >= 0.0) || isinf(p[s]));
        const double total = running_sums<SLOTS>(p, nslots, lane, run);
        if (__ballot(refuse) != 0ull || !(total > 0.0) || isinf(total)) { bad = true; break; }

        const double uu = uw ? uw[k - 1] : uniform53(seed, (uint32_t)b, (uint32_t)r, (uint32_t)(k - 1));
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

    int32_t *out = tours + walk * (size_t)(n + 1);
#pragma unroll
    for (int s = 0; s <= SLOTS; ++s) {
        const int k = lane + kLanes * s;
        if (k <= n) out[k] = bad ? -1 : t[s];
    }
    if (lane == 0) status[walk] = bad ? GNNGLS_SAMPLE_BAD_WEIGHTS_DEV : 0;
}

template <int SLOTS>
hipError_t launch(const double *W, size_t walks, int n, int R, int depot, int invert, uint64_t seed, const double *u,
                  int32_t *tours, int32_t *status, hipStream_t stream) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(sample_nn_kernel<SLOTS>, dim3((unsigned)walks), dim3(kLanes), 0, stream, W, n, R, depot, invert, seed, u, tours,
                       status);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_sample_nn_tours(const double *W, int B, int n, int R, int depot, int invert, uint64_t seed, const double *u,
                                  int32_t *tours, int32_t *status, hipStream_t stream) {
    const size_t walks = (size_t)B * (size_t)R;
    if (walks == 0) return hipSuccess;
    const int nslots = (n + kLanes - 1) / kLanes;        // instantiations: 1, 2, 4, 8, 16 nodes per lane
    if (nslots <= 1) return launch<1>(W, walks, n, R, depot, invert, seed, u, tours, status, stream);
    if (nslots <= 2) return launch<2>(W, walks, n, R, depot, invert, seed, u, tours, status, stream);
    if (nslots <= 4) return launch<4>(W, walks, n, R, depot, invert, seed, u, tours, status, stream);
    if (nslots <= 8) return launch<8>(W, walks, n, R, depot, invert, seed, u, tours, status, stream);
    return launch<16>(W, walks, n, R, depot, invert, seed, u, tours, status, stream);
}

}  // namespace gnngls
