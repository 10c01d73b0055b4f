// model_plan.h -- the regret model's forward, and its training step, each as one value made by one pure function: the layout of the
// packed weights and of the workspace, the refusals, and which kernels run in which form and launch shape.  capi.hip makes the
// request and executes the plan; the launchers of model_kernels.hip / heads_kernels.hip / train_kernels.hip take what it decided.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "model_policy.h"

namespace gnngls {

// ---- the packed weight image (and, same layout, its gradients): float offsets; models.py:20-36 ---------------------------------
struct LayerOffsets { long fc_w, attn_l, attn_r, bn1_g, bn1_b, w1, b1, w2, b2, bn2_g, bn2_b; };
struct PackedModel {
    long emb_w, emb_b, layers, layer_floats, dec_w, dec_b, total;
    LayerOffsets layer(int l) const;
};
PackedModel packed_model(int in_dim, int n_layers);

// ---- the prepared image (gnngls_regret_prepare): byte offsets of layer l's feed-forward weights in bf16 pieces and, behind the
// layers, of A = We^T Wfc^T and b' = Wfc be of the fused embed + first fc; the size with 256 bytes of alignment slack ---------------
constexpr size_t prepared_layer(int l) { return (size_t)l * kFfnPackedBytes; }
constexpr size_t prepared_embed_fc(int n_layers) { return prepared_layer(n_layers); }
constexpr size_t prepared_bytes(int n_layers) { return prepared_embed_fc(n_layers) + kEmbedFcBytes + 256; }

// ---- the forward's workspace for M = (instances of a chunk) x N rows: byte offsets from its 256-byte aligned base ----------------
struct ForwardLayout { size_t h, ft, part, part_ms, h2, hms, end; };     // h / h2 ping-pong; hms (16 heads only): [2][M][32]
ForwardLayout forward_layout(long M, int n_heads);

// ---- experiment switches (A/B runs), read from the environment by capi.hip once per process ------------------------------------
struct ForwardSwitches {
    bool ffn_fp32 = false;     // GNNGLS_FFN_FP32: the feed-forward block on the fp32 matrix pipe, as without a prepared image
    int rank1_mode = -1;       // GNNGLS_GAT_RANK1: -1 default, 0 no rank-1 first GATConv, 2 rank-1 but h_0 and 128-wide partials kept
    int gat_heads = 0;         // GNNGLS_GAT_HEADS: 0 policy, 4 or 8 heads per K1 workgroup
};

enum EmbedForm { EMBED_NONE, EMBED_PLAIN, EMBED_FC, EMBED_FC_H_ONLY };    // _H_ONLY: no ft written (rank-1 first GATConv)
enum AttnForm { ATTN_RANK1, ATTN_RANK1_COMPACT, ATTN_K1, ATTN_K1H };
struct AttnStep {
    AttnForm form;
    int heads_per_wg, waves; size_t lds;
    int F;                     // K1h: features per head
    bool merge16;              // K1h with 16 heads: gat_heads_merge16_kernel follows in the same span
};
struct FfnStep {
    bool bf16x3;               // else the fp32 kernel, which knows none of the forms below
    bool writes_next_ft;       // the next layer's ft = fc(h) from the same launch
    bool decision;             // the decision layer folded into the epilogue: y_out written, the layer's output not stored
    bool rank1_input;          // input formed from the one feature and the compact partials of ATTN_RANK1_COMPACT
};
struct LayerStep { bool fc_launch; AttnStep attn; FfnStep ffn; };
AttnStep gat_rows_step(int n, int forced_heads);       // K1
AttnStep gat_heads_rows_step(int n, int n_heads);      // K1h

enum ForwardRefusal { FWD_OK, FWD_BAD_HEADS, FWD_BAD_ARG, FWD_K1_LDS, FWD_K1H_NODES, FWD_IMAGE_SMALL, FWD_WORKSPACE_SMALL };

struct ForwardRequest {
    int n, B, in_dim, n_layers, n_heads;
    bool pointers_given;       // feat, weights, y_out and workspace are all non-NULL
    bool one_call;             // the caller has no image: the forward builds a scratch image itself if the plan says so
    bool image_given; int64_t image_bytes;
    int64_t workspace_avail;   // bytes behind the workspace's first 256-byte boundary
    ForwardSwitches sw;
};

struct ForwardPlan {
    int status;                // GNNGLS_OK, GNNGLS_ERR_ARG, GNNGLS_ERR_UNSUPPORTED
    ForwardRefusal why;
    int64_t number;            // what the refusal's message prints: LDS bytes, the n limit, or the bytes needed
    bool build_image;          // one-call form: make the scratch image first (also before a later refusal, as ever)
    bool use_image;
    long Bc;                   // instances per chunk (0: nothing to run)
    ForwardLayout ws;          // for Bc * N rows
    EmbedForm embed;
    int n_layers;
    LayerStep first, middle, last;     // layer 0; layers 1 .. n_layers - 2; layer n_layers - 1 where it is not layer 0
    bool decision_launch;
    const LayerStep &layer(int l) const { return l == 0 ? first : l + 1 == n_layers ? last : middle; }
};
ForwardPlan forward_plan(const ForwardRequest &r);

// ---- the training step (forward with batch-statistics BatchNorm + backward) --------------------------------------------------
// Its workspace for M = B * N rows: byte offsets from the 256-byte aligned base, every region a multiple of 256 bytes.  The first
// group is written by the forward and read by the backward (it must survive between the two calls); the second group is scratch.
enum BnSlot { BN_MEAN1, BN_INVSTD1, BN_SCALE1, BN_SHIFT1, BN_MEAN2, BN_INVSTD2, BN_SCALE2, BN_SHIFT2, BN_SLOTS };
enum BatchStatSlot { STAT_MEAN1, STAT_VAR1, STAT_MEAN2, STAT_VAR2, STAT_SLOTS };
// float offset of a layer's slot in the caller's bn_batch_stats [L][4][128]
constexpr size_t batch_stat(int l, BatchStatSlot s) { return ((size_t)l * STAT_SLOTS + s) * kD; }
struct TrainLayout {
    long M;            // rows: B * N
    size_t row;        // bytes of one [M][128] tensor
    int stat_w;        // softmax statistics per node: 16 (one shift and one sum per 16-column slot, H <= 8) or 32 (16 heads: per head)
    size_t H;          // [(L+1)][M][128]  layer inputs (H[0] = embedding) and the final hidden state
    size_t FT;         // [L][M][128]      fc(h)
    size_t G;          // [L][M][128]      GATConv output
    size_t H1;         // [L][M][128]      h + GATConv(h)
    size_t H3;         // [L][M][128]      x + MLP(x), x = BN1(h1)
    size_t HID;        // [L][M][512]      ReLU(W1 x + b1); overwritten by its gradient in the backward
    size_t ATT;        // [L][M][stat_w]   softmax statistics (row max, 1/Z)
    size_t BN;         // [L][BN_SLOTS][128]
    size_t PART;       // [2][M][128]      attention partials (forward) / P partials (backward)
    size_t PMS;        // [2][M][stat_w]   their statistics; 16 heads: per head, where the forward kernel's `hms` points too
    size_t DA, DB;     // [M][128]         gradient ping-pong
    size_t X2;         // [M][128]         BN1 output recomputed in the backward
    size_t DFT;        // [M][128]
    size_t DL, DR;     // [M][stat_w / 2]  d el, d er: the two halves of one region
    size_t W2T, W1T;   // [512*128]        transposed weights of the layer being differentiated: the two halves of one region
    size_t COEF;       // [3][128]         BatchNorm backward coefficients; behind them, in the same region, the constants
    size_t ONES;       // [128]
    size_t ZEROS;      // [512]
    size_t CSP;        // [kColsumMaxBlocks][2][512] doubles: column-sum partials
    size_t TNP;        // [gemm_tn_chunks(M)][128 * 512 + 512]: weight-gradient partial tiles and their column sums
    size_t end;
    size_t h(int l) const { return H + row * l; }
    size_t ft(int l) const { return FT + row * l; }
    size_t g(int l) const { return G + row * l; }
    size_t h1(int l) const { return H1 + row * l; }
    size_t h3(int l) const { return H3 + row * l; }
    size_t hid(int l) const { return HID + 4 * row * l; }
    size_t att(int l) const { return ATT + (size_t)M * stat_w * sizeof(float) * l; }
    size_t bn(int l, BnSlot s) const { return BN + ((size_t)l * BN_SLOTS + s) * kD * sizeof(float); }
};
TrainLayout train_layout(long M, int n_layers, int n_heads);
// gnngls_regret_train_workspace_bytes_heads: the layout's end + 256 bytes of alignment slack; 0 where the ABI gives no size
int64_t train_workspace_bytes(int B, int n, int n_layers, int n_heads);

enum TrainRefusal { TRAIN_OK, TRAIN_BAD_HEADS, TRAIN_BAD_ARG, TRAIN_BWD_NODES, TRAIN_WORKSPACE_SMALL };
// what follows the attention on both ways: slot statistics (gat_combine_train, gat_bwd_combine, CS_HEADSCALE column sums) or the
// per-head forms of 16 heads (gat_heads_merge16_train, gat_heads_bwd_combine16, colsum_heads16)
enum CombineForm { COMBINE_SLOTS, COMBINE_HEADS16 };
struct AttnBwdStep {
    AttnForm form;             // ATTN_K1: gat_bwd_rows_kernel<tiles>; ATTN_K1H: gat_heads_bwd_rows_kernel<F>
    int tiles, F;
    size_t lds;
    int wgs_per_row, waves;    // the grid is B * n * wgs_per_row workgroups of `waves` wavefronts
};
struct TrainRequest {
    int n, B, in_dim, n_layers, n_heads;
    bool pointers_given;       // feat, params, y_out / grads and workspace are all non-NULL
    int64_t workspace_bytes;
    int gat_heads;             // ForwardSwitches::gat_heads
};
struct TrainPlan {
    int status;                // GNNGLS_OK, GNNGLS_ERR_ARG, GNNGLS_ERR_UNSUPPORTED
    TrainRefusal why;
    int64_t number;            // what the refusal's message prints: the n limit or the bytes needed
    TrainLayout ws;            // for M = B * N rows (ws.M)
    AttnStep attn;             // the same launch shape as the inference forward's
    CombineForm combine;
    AttnBwdStep bwd;
};
TrainPlan train_plan(const TrainRequest &r);

}  // namespace gnngls
