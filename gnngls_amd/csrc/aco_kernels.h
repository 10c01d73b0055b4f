// aco_kernels.h -- internal interface between the MAX-MIN ant system (aco_kernels.hip) and the C ABI (capi.hip).
//
// include/gnngls_hip.h states the definition (gnngls_aco_run); gnngls_amd.host.aco restates it in NumPy.  In short, per instance
// and iteration g = iter0 + t: R ants walk the sampled walk of sampling_kernels.h (depot s, invert = 0) on w_j = tau[i,j] * H[i,j];
// a walk's cost is that of its closed tour rotated to start at node 0, summed left to right; the lowest-index cheapest ant (or,
// on the gb_every schedule, the best tour so far) deposits 1 / cost on its edges after every off-diagonal tau was multiplied by
// 1 - rho, and the result is clamped into [tau_max * min_ratio, tau_max], tau_max = 1 / (rho * best_cost).
//
// UNIFORMS.  u[b,t,a,s], s = 0 .. n-2: the caller's array, or Philox4x32-10 (philox.h) with counter (b, g * R + a, s, 2).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gnngls {

constexpr int kAcoMaxN = 1024;          // 16 nodes per lane, as for the sampled walks
constexpr int kAcoMaxAnts = 256;
constexpr int kAcoMaxWaves = 16;        // ant a runs on wavefront a % min(R, 16)
constexpr int kAcoStatusBadWeights = 6; // GNNGLS_SAMPLE_BAD_WEIGHTS

// dynamic LDS of one workgroup (the wavefronts' best tours, the best tour, succ / pred of the deposit tour, the reduction cells)
size_t aco_lds_bytes(int n, int R);

// D, H, tau [B,n,n]; best_tour [B,n+1], best_cost [B] IN/OUT; u [B,K,R,n-1] or NULL; iters_done, status [B]; trace_cost [B,K],
// ant_tours [B,R,n+1], ant_cost [B,R] or NULL.  3 <= n <= kAcoMaxN, 1 <= R <= kAcoMaxAnts, B >= 1.
hipError_t launch_aco(const double *D, const double *H, double *tau, int32_t *best_tour, double *best_cost, int B, int n, int R, int K,
                      long long iter0, double rho, double min_ratio, int gb_every, int spread_starts, uint64_t seed, const double *u,
                      int32_t *iters_done, int32_t *status, double *trace_cost, int32_t *ant_tours, double *ant_cost,
                      hipStream_t stream);

}  // namespace gnngls
