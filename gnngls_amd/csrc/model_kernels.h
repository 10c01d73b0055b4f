// model_kernels.h -- internal interface between the GNN forward kernels (model_kernels.hip) and capi.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gnngls {

enum { GEMM_EPI_STORE = 0, GEMM_EPI_BIAS_RELU = 1, GEMM_EPI_BIAS_SKIP_BN = 2, GEMM_EPI_MASK = 3, GEMM_EPI_ADD = 4 };

struct FfnStep;       // model_plan.h
hipError_t launch_pack_features(const double *D, int B, int n, double scale, double minv, float *feat, hipStream_t st);
hipError_t launch_unpack_regret(const float *y, int B, int n, double scale, double minv, double *out, hipStream_t st);
hipError_t launch_embed(const float *x, const float *W, const float *b, float *h, long M, int in_dim, hipStream_t st);
// embed + the first layer's fc as one rank-in_dim pass (in_dim <= kEmbedFcMaxIn); `image`: kEmbedFcBytes of device memory
hipError_t launch_embed_fc_prepare(const float *We, const float *be, const float *Wfc, const float *attn_l, const float *attn_r,
                                   int in_dim, void *image, hipStream_t st);
// in_dim == 1: the first GATConv from the one input feature and the same image (partials as launch_gat_rows on ft = x A + b')
// compact: [2][B N][24] = (shift, sum of weights, sum of weights x feature) per head into `part` (for launch_ffn_fused's lr_img form)
hipError_t launch_gat_rows_rank1(const float *x, const void *image, int B, int n, float *part, float *part_ms, hipStream_t st,
                                 bool compact = false);
hipError_t launch_embed_fc(const float *x, const float *W, const float *b, const void *image, float *h, float *ft, long M, int in_dim,
                           hipStream_t st);
hipError_t launch_gemm(int epi, const float *A, const float *W, float *C, long M, int N, int K, const float *bias,
                       const float *skip, const float *bn_scale, const float *bn_shift, hipStream_t st);
// C[M,N] = A[M,K] * W[K,N] (W row-major [K,N]); epi STORE / MASK (C = acc * (aux > 0)) / ADD (C = acc + aux)
hipError_t launch_gemm_wkn(int epi, const float *A, const float *W, float *C, long M, int N, int K, const float *aux,
                           hipStream_t st);
hipError_t launch_ffn_fused_train(const float *h1, const float *bn1_s, const float *bn1_b, const float *W1, const float *b1,
                                  const float *W2, const float *b2, const float *ones, const float *zeros, float *h3,
                                  float *hidden, long M, hipStream_t st);
hipError_t launch_ffn_fused_bwd(const float *dh3, const float *W2T, const float *W1T, const float *ones, const float *zeros,
                                float *dx, float *hidden, long M, hipStream_t st);
hipError_t launch_transpose_pair(const float *W2, const float *W1, float *W2T, float *W1T, hipStream_t st);
hipError_t launch_gat_rows(const float *ft, const float *attn_l, const float *attn_r, int B, int n, int heads_per_wg, int waves,
                           float *part, float *part_ms, hipStream_t st);
// the operands of launch_ffn_fused; which of the tail it reads is the FfnStep's business
struct FfnFused {
    const float *part, *part_ms, *hin, *bn1_s, *bn1_b, *W1, *b1, *W2, *b2, *bn2_s, *bn2_b;
    float *hout; long M;
    const void *packed;                        // bf16x3: the layer's image (kFfnPackedBytes, launch_ffn_pack)
    float *ft_out;                             // writes_next_ft
    const float *dec_w, *dec_b; float *y_out;  // decision
    const float *lr_img, *emb_w, *emb_b;       // rank1_input: the embed-fc image and the embedding
};
hipError_t launch_ffn_fused(const FfnFused &a, const FfnStep &form, hipStream_t st);
hipError_t launch_ffn_pack(const float *W1, const float *W2, const float *fc_next, void *packed, hipStream_t st);
hipError_t launch_decision(const float *h, const float *w, const float *b, float *y, long M, hipStream_t st);

}  // namespace gnngls
