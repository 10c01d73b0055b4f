// threeopt_kernels.h -- internal interface between the 3-opt kernels (threeopt_kernels.hip) and the C ABI (capi.hip).
//
// 3-opt removes the tour edges at three positions p1 < p2 < p3 and reconnects the pieces B = t[p1+1..p2] and C = t[p2+1..p3]
// between the head and the tail in the four ways that are no 2-opt move (kind 0..3).  The candidate (p1, p2, p3, kind), its delta
// in the stated operand order, the enumeration order and the descent (local_search, algorithms.py:111-132, with relocate_a2a
// replaced by the 3-opt scan) are the contract stated in include/gnngls_hip.h.  One workgroup per instance, one launch per batch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gnngls {

// a move's selection key holds its three positions in eight bits each and the kind in two
constexpr int kThreeOptMaxN = 256;
constexpr int kThreeOptStatusAsymmetric = 3;   // GNNGLS_STATUS_ASYMMETRIC
constexpr int kThreeOptStatusMoveCap = 6;      // GNNGLS_STATUS_MOVE_CAP

// tour [B,n+1], D [B,n,n] -> delta [B] (0.0: no move; NaN: the matrix is not bitwise symmetric), move [B,4] = p1, p2, p3, kind
// (-1s when none), new_tour [B,n+1] (the input when none).  3 <= n <= kThreeOptMaxN, B >= 1.
hipError_t launch_three_opt_best_move(const int32_t *tour, const double *D, int B, int n, double *delta, int32_t *move,
                                      int32_t *new_tour, hipStream_t stream);

// the descent: tour [B,n+1], cost [B], D [B,n,n] -> tour_out, cost_out, moves [B], status [B], trace_cost [B,trace_cap] or NULL
// (the cost after every applied move, the first trace_cap of them).  max_moves >= 1 bounds the loop.
hipError_t launch_three_opt_descent(const int32_t *tour, const double *cost, const double *D, int B, int n, int max_moves,
                                    int32_t *tour_out, double *cost_out, int32_t *moves, int32_t *status, double *trace_cost,
                                    int trace_cap, hipStream_t stream);

// workgroup size of the launches for n nodes, their dynamic LDS, and the largest n whose distance triangle is staged in LDS
// (larger instances read D from global memory)
int three_opt_threads(int n);
int three_opt_lds_bytes(int n);
int three_opt_lds_max_n();

}  // namespace gnngls
