// greedy_edge_kernels.h -- internal interface between the greedy edge matching decoder (greedy_edge_kernels.hip) and the C ABI
// (capi.hip).
//
// include/gnngls_hip.h states the definition (gnngls_greedy_edge); gnngls_amd.host.greedy_edge restates it in NumPy.  In short,
// per instance: the undirected edges {i, j}, i < j, in ascending (S[i,j], i, j) -- a zero key taken as +0.0 --; an edge is accepted
// if both ends have degree below 2 and are not the two ends of one path fragment; after n - 1 acceptances the two nodes of degree
// 1 are joined; the tour is read from `depot` towards the smaller-numbered of its two neighbours.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gnngls {

constexpr int kGreedyEdgeMaxN = 1024;            // one thread per node in the acceptance step; an edge packs (i, j) into 16 + 16 bits
constexpr int kGreedyEdgeMaxWaves = 16;          // the workgroup has min(ceil(n / 16), 16) wavefronts, never fewer threads than nodes
constexpr int kGreedyEdgeStatusBadScore = 1;     // GNNGLS_GREEDY_EDGE_BAD_SCORE
constexpr int kGreedyEdgeStatusStalled = 2;      // GNNGLS_GREEDY_EDGE_STALLED

// wavefronts and dynamic LDS of one workgroup (44 B per node and a few words: 45,104 B at n = 1024)
int greedy_edge_waves(int n);
size_t greedy_edge_lds_bytes(int n);

// S [B,n,n]; D [B,n,n] or NULL; tour [B,n+1]; score, cost [B]; edges [B,n,2] or NULL; rounds, status [B].
// 3 <= n <= kGreedyEdgeMaxN, 0 <= depot < n, B >= 1.  No global workspace.
hipError_t launch_greedy_edge(const double *S, const double *D, int B, int n, int depot, int32_t *tour, double *score, double *cost,
                              int32_t *edges, int32_t *rounds, int32_t *status, hipStream_t stream);

}  // namespace gnngls
