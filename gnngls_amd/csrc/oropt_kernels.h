// oropt_kernels.h -- internal interface between the Or-opt kernels (oropt_kernels.hip) and the C ABI (capi.hip).
//
// Or-opt moves a chain of one to three consecutive tour nodes between two other tour neighbours, forward or reversed; with chains
// of one node and no reversal it is the reference's relocate (operators.py:76-147).  The candidate (i, L, rev, j), its delta in
// the reference's operand order, the enumeration order and the descent (local_search, algorithms.py:111-132, with relocate_a2a
// replaced by the Or-opt scan) are the contract stated in include/gnngls_hip.h.  One workgroup per instance, one launch per batch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gnngls {

// a move's selection key holds i and j in ten bits each
constexpr int kOrOptMaxN = 1024;
constexpr int kOrOptMaxSeg = 3;
constexpr int kOrOptStatusAsymmetric = 3;      // GNNGLS_STATUS_ASYMMETRIC
constexpr int kOrOptStatusMoveCap = 6;         // GNNGLS_STATUS_MOVE_CAP
constexpr int kGuidedStatusStepCap = 7;        // GNNGLS_STATUS_STEP_CAP

// tour [B,n+1], D [B,n,n] -> delta [B] (0.0: no move; NaN: the matrix is not bitwise symmetric), move [B,4] = i, L, rev, j (-1s
// when none), new_tour [B,n+1] (the input when none).  3 <= n <= kOrOptMaxN, 1 <= max_seg <= kOrOptMaxSeg, B >= 1.
hipError_t launch_or_opt_best_move(const int32_t *tour, const double *D, int B, int n, int max_seg, int reverse, double *delta,
                                   int32_t *move, int32_t *new_tour, hipStream_t stream);

// the descent: tour [B,n+1], cost [B], D [B,n,n] -> tour_out, cost_out, moves [B], status [B], trace_cost [B,trace_cap] or NULL
// (the cost after every applied move, the first trace_cap of them).  max_moves >= 1 bounds the loop.
hipError_t launch_or_opt_descent(const int32_t *tour, const double *cost, const double *D, int B, int n, int max_seg, int reverse,
                                 int max_moves, int32_t *tour_out, double *cost_out, int32_t *moves, int32_t *status,
                                 double *trace_cost, int trace_cap, hipStream_t stream);

// iterated local search (the contract is in include/gnngls_hip.h): the descent above, then `kicks` times a double-bridge kick of
// the accepted tour, a descent of the kicked tour, and the better of the two kept.  u [B,kicks,3] uniforms or NULL (Philox,
// counter (b, kick0 + k, s, 1)); trace_cost [B,kicks] or NULL: the candidate's cost after every kick.  4 <= n <= kOrOptMaxN,
// kicks >= 0, kick0 >= 0, max_moves >= 1 bounds the applied moves of the whole run.
hipError_t launch_ils(const int32_t *tour, const double *cost, const double *D, int B, int n, int kicks, int kick0, int max_seg, int reverse,
                      int max_moves, uint64_t seed, const double *u, int32_t *tour_out, double *cost_out, int32_t *moves,
                      int32_t *accepted, int32_t *status, double *trace_cost, hipStream_t stream);

// the one-to-all scan: the outputs of launch_or_opt_best_move over the candidates (s, L, rev, j) whose chain t[s .. s+L-1] holds
// position pos[b] (pos [B]; a position outside 1..n-1 has no candidates).  3 <= n <= kOrOptMaxN.
hipError_t launch_or_opt_o2a(const int32_t *tour, const double *D, const int32_t *pos, int B, int n, int max_seg, int reverse,
                             double *delta, int32_t *move, int32_t *new_tour, hipStream_t stream);

// guided local search over 2-opt and Or-opt (the contract is in include/gnngls_hip.h): the descent above, then outer_iters times
// penalty steps (one-to-all scans on D + k * penalty) until perturbation_moves moves are applied, the descent, the better tour
// kept.  guides [G,B,n,n] (NULL only with outer_iters 0), k [B], penalty [B,n,n] int32 symmetric IN/OUT; trace_cost
// [B,trace_cap] or NULL, trace_len [B] or NULL.  4 <= n <= kOrOptMaxN; max_moves >= 1 and max_steps >= 1 bound the run.
hipError_t launch_guided_or_opt(const int32_t *tour, const double *cost, const double *D, const double *guides, int G, const double *k,
                                int32_t *penalty, int B, int n, int outer_iters, int iter0, int perturbation_moves, int max_seg,
                                int reverse, int max_moves, int max_steps, int32_t *tour_out, double *cost_out, int32_t *best_tour,
                                double *best_cost, int32_t *moves, int32_t *steps, int32_t *status, double *trace_cost, int trace_cap,
                                int32_t *trace_len, hipStream_t stream);
int guided_or_opt_lds_bytes(int n);

// workgroup size of the launches for n nodes (one wavefront per 16 nodes, sixteen at most) and their dynamic LDS
int or_opt_threads(int n);
int or_opt_lds_bytes(int n);

}  // namespace gnngls
