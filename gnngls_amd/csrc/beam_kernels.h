// beam_kernels.h -- internal interface between the beam-search decoder (beam_kernels.hip) and the C ABI (capi.hip).
//
// include/gnngls_hip.h states the definition (gnngls_beam_search); gnngls_amd.host.beam_search restates it in NumPy.  In short,
// per instance: beams are paths from `depot` with a score c; step t = 1 .. n-1 forms every (beam k, unvisited node j) with the
// key c_k + S[last_k, j] (one add, a zero taken as +0.0) and keeps the min(width, #candidates) smallest in (key, k, j), ranked in
// that order; the close adds S[last, depot]; the best beam is the smallest in (score, rank) or in (cost on D, rank).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gnngls {

constexpr int kBeamMaxN = 1024;          // a back-pointer packs (parent rank, node) into 10 + 10 bits
constexpr int kBeamMaxWidth = 1024;
constexpr int kBeamMaxWaves = 16;        // the workgroup has min(width, 16) wavefronts; beam k is scanned by wavefront k % 16
constexpr int kBeamStatusBadScore = 1;   // GNNGLS_BEAM_BAD_SCORE
// The LDS one workgroup may take: half of the 160 KiB of a CU, so that LDS never keeps a second workgroup off a CU (at 128 VGPRs
// a CU holds 16 wavefronts, so today only workgroups of at most 8 wavefronts, width <= 8, share one).  The visited bitmasks
// (2 * width * ceil(n / 64) words) live in LDS where everything fits under this, else in the global workspace.
constexpr size_t kBeamLdsBudget = 80 * 1024;

// dynamic LDS of one workgroup, the bitmasks included where beam_masks_in_lds(n, width)
size_t beam_lds_bytes(int n, int width);
bool beam_masks_in_lds(int n, int width);
// the global workspace of a batch: per instance the back-pointers [(n-1), width] uint32, a [width, n+1] int32 tour buffer and,
// where the bitmasks do not fit into LDS, 2 * width * ceil(n / 64) uint64
size_t beam_workspace_bytes(int B, int n, int width);

// S [B,n,n]; D [B,n,n] or NULL; best_tour [B,n+1]; best_score, best_cost [B]; n_beams, status [B]; beam_tours [B,width,n+1],
// beam_score, beam_cost [B,width] or all NULL; workspace of beam_workspace_bytes(B, n, width) bytes, 16-byte aligned.
// 3 <= n <= kBeamMaxN, 1 <= width <= kBeamMaxWidth, 0 <= depot < n, select_cost implies D, B >= 1.
hipError_t launch_beam_search(const double *S, const double *D, int B, int n, int width, int depot, int select_cost, int32_t *best_tour,
                              double *best_score, double *best_cost, int32_t *n_beams, int32_t *status, int32_t *beam_tours,
                              double *beam_score, double *beam_cost, void *workspace, hipStream_t stream);

}  // namespace gnngls
