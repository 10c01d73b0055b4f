// sampling_kernels.h -- internal interface between the sampled nearest-neighbour walks (sampling_kernels.hip) and the C ABI
// (capi.hip).
//
// Walk (b, r) restates probabilistic_nearest_neighbour (algorithms.py:21-50) with the uniforms as an explicit input:
//   tour = [depot]; at every step i = tour[-1], the candidates are the unvisited nodes j in ascending id with g_j = W[b,i,j];
//   p = g;  if any g_j is +-inf: p_j = 1.0 where g_j is infinite, 0.0 elsewhere (:34-36);
//   if sum(p) == 0: every p_j = 1.0 (:39-40);  if invert: p_j = 1 / p_j (:43-44);
//   where np.random.choice would raise -- some p_j NaN, negative or infinite, or the total not finite and positive -- the walk
//   stops: status GNNGLS_SAMPLE_BAD_WEIGHTS_DEV, its tour row filled with -1;
//   draw: x = u * total; the first candidate with p_j > 0 whose running sum exceeds x; if rounding leaves none, the last
//   candidate with p_j > 0.  (A candidate with p_j = 0 can be the first to exceed x only through rounding; it is never picked.)
//
// SUMMATION ORDER (part of the definition: it decides ties at a boundary).  Node j sits on lane j % 64, slot j / 64; a node that
// is no candidate (visited, or >= n) contributes +0.0.  For slot s = 0, 1, .. in order:
//   c_s     = the inclusive doubling scan of slot s over the 64 lanes: for d = 1, 2, 4, 8, 16, 32 in order, every lane l >= d adds
//             the value lane l - d held BEFORE this round (Hillis-Steele);
//   run_j   = base_s + c_s[lane of j]      with base_0 = +0.0, base_{s+1} = base_s + c_s[63];
//   total   = base after the last slot that holds a node (slots beyond add +0.0 and change nothing).
// sum(p) of the all-zero rule is `total` of this scheme on the p before inversion.  Every operation is one fp64 add, multiply or
// divide, rounded once (the unit is compiled with contraction off).
//
// UNIFORMS.  u[b,r,s] in [0,1), s = 0 .. n-2 (the last step, with one candidate, draws too, as the reference does): the caller's
// array, or Philox4x32-10 with key (seed & 0xffffffff, seed >> 32) and counter (b, r, s, 0): u = ((out0 << 32 | out1) >> 11) * 2^-53.
// A u outside [0,1) (or NaN) still gives a closed permutation; which one is unspecified.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define GNNGLS_SAMPLE_BAD_WEIGHTS_DEV 6

namespace gnngls {

constexpr int kSampleMaxN = 1024;       // 16 nodes per lane: visited bits and candidate weights stay in registers

// W [B,n,n]; u [B,R,n-1] or NULL (Philox, keyed by seed); tours [B,R,n+1]; status [B,R].  3 <= n <= kSampleMaxN, B * R walks.
hipError_t launch_sample_nn_tours(const double *W, int B, int n, int R, int depot, int invert, uint64_t seed, const double *u,
                                  int32_t *tours, int32_t *status, hipStream_t stream);

}  // namespace gnngls
