// bounds_kernels.h -- internal interface between the Held-Karp 1-tree lower bound (bounds_kernels.hip) and the C ABI (capi.hip).
//
// The bound is the far side of the gap the reference reports against Concorde's optimum (scripts/test.py:62,104,
// gnngls/__init__.py:55-60): for node potentials pi, w(pi) = min 1-tree of c + pi_i + pi_j  -  2 sum(pi)  <=  optimum, and the
// subgradient ascent of oracle/one_tree.c (one_tree_lower_bound with min_one_tree) returns max_k w(pi_k).  The kernel repeats
// that file's fp64 operations in its order: same bits.  One workgroup per instance, the whole ascent in one launch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define GNNGLS_STATUS_ASYMMETRIC_DEV 3

namespace gnngls {

// a node's key, parent, potential, best potential and degree live in registers (at most four nodes per lane, at most four
// wavefronts per instance); sum (deg - 2)^2 <= (2n)^2 = 2^22 fits 32 bits
constexpr int kOneTreeMaxN = 1024;

enum { BOUND_EXIT_ITERS = 0, BOUND_EXIT_STEP = 1, BOUND_EXIT_TOUR = 2 };

// D [B,n,n], ub [B]; bound [B], pi [B,n] or NULL, iters [B], exit_kind [B], status [B].  3 <= n <= kOneTreeMaxN, B >= 1.
hipError_t launch_one_tree_bound(const double *D, const double *ub, int B, int n, int max_iters, double *bound, double *pi,
                                 int32_t *iters, int32_t *exit_kind, int32_t *status, hipStream_t stream);

// workgroup size of the launch for n nodes (64: one wavefront, n <= 256) and its dynamic LDS
int one_tree_threads(int n);
int one_tree_lds_bytes(int n);

}  // namespace gnngls
