// labels_kernels.h -- internal interface between the regret-label kernels (labels_kernels.hip) and the C ABI (capi.hip).
//
// A fixed-edge job is one instance b plus one edge (i, j) that is not on b's base tour.  Its search is the reference's
// guided_local_search (algorithms.py:135-195) on the instance with one changed weight, w'(i,j) = w'(j,i) = fl(D[i,j] - M_b),
// guides = ['weight'] on that matrix, started from the base tour.  M_b = the smallest power of two >= (2 n) max(D_b): every
// tour with the edge is cheaper under D' than every tour without it, so the search keeps the edge once it has inserted it.
// The label is the true cost of the returned tour (tour_cost on D, gnngls/__init__.py:17-21); datasets.py:23-34 turns it into
// regret = (cost - base_cost) / base_cost.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define GNNGLS_STATUS_EDGE_LOST_DEV 4

namespace gnngls {

// one job: instance, the two endpoints (i < j) and the line-graph index r(i, j) of the edge
struct LabelJob { int32_t inst, i, j, r; };

// rank of (i < j) in itertools.combinations(range(n), 2) order = the line-graph node of the edge (models.LineGraph)
__host__ __device__ inline int edge_rank(int i, int j, int n) { return i * n - i * (i + 1) / 2 + (j - i - 1); }

// M_b of every instance: smallest power of two >= (2.0 * n) * max(D_b) (1.0 if that product is not > 0)
hipError_t launch_label_offsets(const double *D, int B, int n, double *offset, hipStream_t stream);
// best_* = the base tour (rank -1, cost base_cost[b]); status = 0; edge_cost = +inf unless keep_edge_cost
hipError_t launch_label_init(int B, int n, const int32_t *base_tour, const double *base_cost, bool keep_edge_cost,
                             double *edge_cost, double *best_cost, int32_t *best_rank, int32_t *best_tour, int32_t *status,
                             hipStream_t stream);
// per job: D' [J,n,n] (also the guide) and the start tour [J,n+1] (the instance's base tour)
hipError_t launch_label_expand(const double *D, int n, const int32_t *base_tour, const LabelJob *jobs, int J, const double *offset,
                               double *Dp, int32_t *tours, hipStream_t stream);
// per job: true cost of the returned tour on D, check that it holds (i, j), then edge_cost[inst, r] = min(edge_cost, cost);
// jobs whose search status is PENALTY_OVERFLOW are skipped (the caller reruns them); then per instance of the chunk the
// cheapest tour by (cost, rank) replaces best_* if it beats it
hipError_t launch_label_collect(const double *D, int n, const LabelJob *jobs, int J, const int32_t *tours, const int32_t *job_status,
                                double *job_cost, double *edge_cost, double *best_cost, int32_t *best_rank, int32_t *best_tour,
                                int32_t *status, hipStream_t stream);
// base edges: edge_cost = base_cost and regret = 0.0 exactly; other edges: regret = (edge_cost - base_cost) / base_cost
hipError_t launch_label_finalize(int B, int n, const int32_t *base_tour, const double *base_cost, double *edge_cost, double *regret,
                                 hipStream_t stream);

}  // namespace gnngls
