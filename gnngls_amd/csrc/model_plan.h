// model_plan.h -- the regret model's forward as one value made by one pure function: the layout of the packed weights and of the
// workspace, the refusals, and which kernels run in which form and launch shape.  capi.hip makes the request and executes the plan;
// the launchers of model_kernels.hip / heads_kernels.hip take what the plan decided.
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

}  // namespace gnngls
