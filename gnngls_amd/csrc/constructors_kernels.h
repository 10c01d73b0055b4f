// constructors_kernels.h -- internal interface between the insertion tour constructors (constructors_kernels.hip) and the
// C ABI (capi.hip).
//
// insertion (algorithms.py:82-108) grows the closed tour [depot, depot] by one node per step: the next node is the nearest /
// farthest outside node to any tour member (algorithms.py:93-103) or the next entry of a caller's order (the host's
// np.random.choice draws, algorithms.py:90-91); cheapest_insertion (algorithms.py:67-79) puts it where tour_cost
// (gnngls/__init__.py:17-21: the left-to-right fp64 sum over ALL edges of the candidate tour) is strictly smallest, first
// position on ties.  One workgroup per instance, the whole construction in one launch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define GNNGLS_STATUS_BAD_ORDER_DEV 5

namespace gnngls {

enum { INSERT_NEAREST = 0, INSERT_FARTHEST = 1, INSERT_GIVEN_ORDER = 2 };

// largest n of both entries: 48 B of LDS per node (two tours, two edge-weight arrays, prefix sums, per-node extreme / member /
// position) -> 98 KiB at n = 2048
constexpr int kInsertionMaxN = 2048;

// tour_out [B,n+1]; order [B,n-1] and status [B] for INSERT_GIVEN_ORDER (status may be NULL otherwise)
hipError_t launch_insertion(const double *W, int B, int n, int depot, int mode, const int32_t *order, int32_t *tour_out,
                            int32_t *status, hipStream_t stream);
// sub_tour [B,len] closed sub-tours, node [B]; tour_out [B,len+1], cost_out [B] (NaN and an untouched tour row where an index
// is out of 0..n-1)
hipError_t launch_cheapest_insertion(const int32_t *sub_tour, int len, const int32_t *node, const double *W, int B, int n,
                                     int32_t *tour_out, double *cost_out, hipStream_t stream);

}  // namespace gnngls
