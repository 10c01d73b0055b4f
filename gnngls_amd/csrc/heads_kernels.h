// heads_kernels.h -- internal interface between the attention kernels for head counts other than 8 (heads_kernels.hip) and capi.hip.
// embed_dim 128: H in {1, 2, 4, 16} heads of F = 128 / H features; n <= kMaxNodes (model_policy.h) for every launcher here.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gnngls {

// attention partials of every row: `part` [2][B N][128] by side; statistics into part_ms [2][B N][8 + 8] per 16-column slot
// (H <= 4) or into hms [2][B N][16 + 16] per head (H = 16, then launch_gat_heads_merge16 before the feed-forward launch);
// waves: gat_heads_rows_step() of the plan
hipError_t launch_gat_heads_rows(const float *ft, const float *attn_l, const float *attn_r, int B, int n, int n_heads, int waves,
                                 float *part, float *part_ms, float *hms, hipStream_t st);
// H = 16: the merged GATConv output into part side 0 (side 1 zero) with neutral statistics in part_ms (inference) ...
hipError_t launch_gat_heads_merge16(float *part, const float *hms, float *part_ms, long M, hipStream_t st);
// ... or g, h1 = h + g and att [M][16 + 16] (row max, 1/Z per head) for the training step
hipError_t launch_gat_heads_merge16_train(const float *part, const float *hms, const float *h, long M, float *g, float *h1, float *att,
                                          hipStream_t st);
// GATConv backward: P [2][B N][128]; d el / d er into dlr [2][B N][8 + 8] per slot (H <= 4: launch_gat_bwd_combine) or
// [2][B N][16 + 16] per head (H = 16: launch_gat_heads_bwd_combine16); att in the layout its forward wrote; lds: the plan's
// (gat_heads_bwd_lds_bytes of model_policy.h)
hipError_t launch_gat_heads_bwd_rows(const float *ft, const float *dout, const float *gout, const float *att, const float *attn_l,
                                     const float *attn_r, int B, int n, int n_heads, size_t lds, float *P, float *dlr, hipStream_t st);
hipError_t launch_gat_heads_bwd_combine16(const float *P, const float *dlr, const float *attn_l, const float *attn_r, long M,
                                          float *dft, float *dl, float *dr, hipStream_t st);
// H = 16: the attn_l / attn_r gradient column sums (dl / dr [M][16]) into colsum partials of nblocks = colsum_blocks(M, 128)
hipError_t launch_colsum_heads16(const float *X, const float *Y, const float *Y2, long M, double *partial, int nblocks,
                                 hipStream_t st);

}  // namespace gnngls
