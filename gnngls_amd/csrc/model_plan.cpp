// model_plan.cpp -- the plans of the regret forward and of the training step: plain host C++ (no HIP call, no global, no environment), see model_plan.h.
#include "model_plan.h"

#include "../../include/gnngls_hip.h"

namespace gnngls {

namespace {
constexpr long kFfnHidden = 4 * kD;      // models.py:28
LayerOffsets layer_at(long base) {
    LayerOffsets p;
    p.fc_w = base; p.attn_l = p.fc_w + (long)kD * kD; p.attn_r = p.attn_l + kD; p.bn1_g = p.attn_r + kD; p.bn1_b = p.bn1_g + kD;
    p.w1 = p.bn1_b + kD; p.b1 = p.w1 + kFfnHidden * kD; p.w2 = p.b1 + kFfnHidden; p.b2 = p.w2 + kD * kFfnHidden; p.bn2_g = p.b2 + kD;
    p.bn2_b = p.bn2_g + kD;
    return p;
}
}  // namespace

LayerOffsets PackedModel::layer(int l) const { return layer_at(layers + (long)l * layer_floats); }

PackedModel packed_model(int in_dim, int n_layers) {
    PackedModel m;
    m.emb_w = 0; m.emb_b = (long)kD * in_dim; m.layers = m.emb_b + kD;
    m.layer_floats = layer_at(0).bn2_b + kD;
    m.dec_w = m.layers + (long)n_layers * m.layer_floats; m.dec_b = m.dec_w + kD;
    m.total = m.dec_b + 4;                                   // (the decision bias padded to 16 bytes)
    return m;
}

ForwardLayout forward_layout(long M, int n_heads) {
    const size_t row = (size_t)M * kD * sizeof(float);
    ForwardLayout w;
    w.h = 0; w.ft = w.h + row; w.part = w.ft + row;           // part [2][M][128], part_ms [2][M][16]
    w.part_ms = w.part + 2 * row; w.h2 = w.part_ms + (size_t)2 * M * 16 * sizeof(float);
    w.hms = w.h2 + row;
    // 16 heads: + the per-head softmax statistics of both sides [2][16 + 16] per row (gat_heads_merge16_kernel's input)
    w.end = w.hms + (n_heads == 16 ? (size_t)M * 2 * 32 * sizeof(float) : 0);
    return w;
}

AttnStep gat_rows_step(int n, int forced_heads) {
    const int hs = forced_heads ? forced_heads : gat_rows_heads(n);
    const size_t lds = gat_rows_lds_bytes_hs(n, hs);
    return {ATTN_K1, hs, gat_rows_waves(gat_rows_units(n, hs), lds), lds, kF, false};
}

AttnStep gat_heads_rows_step(int n, int n_heads) {
    const int F = kD / n_heads;
    return {ATTN_K1H, (n_heads == 1 ? kD : 64) / F, gat_heads_rows_waves(gat_heads_rows_units(n, n_heads)),
            gat_heads_rows_lds_bytes(n, n_heads), F, n_heads == 16};
}

ForwardPlan forward_plan(const ForwardRequest &r) {
    ForwardPlan p{};
    p.status = GNNGLS_OK; p.why = FWD_OK; p.n_layers = r.n_layers;
    auto refuse = [&p](int status, ForwardRefusal why, int64_t number) { p.status = status; p.why = why; p.number = number; return p; };
    if (!heads_supported(r.n_heads)) return refuse(GNNGLS_ERR_UNSUPPORTED, FWD_BAD_HEADS, r.n_heads);
    if (r.B == 0) return p;    // empty batch: nothing to enqueue (data pointers may be NULL)
    if (!r.pointers_given || r.B < 0 || r.n < 3 || r.in_dim < 1 || r.n_layers < 0) return refuse(GNNGLS_ERR_ARG, FWD_BAD_ARG, 0);
    const bool h8 = r.n_heads == 8, beyond_k1h = !h8 && r.n > kMaxNodes;
    // the one-call form splits the weights into scratch of its own unless the feed-forward stays on the fp32 pipe, there is no
    // layer, or the head count refuses this n (the 8-head and the workspace refusals come after the image, as ever)
    p.build_image = r.one_call && !beyond_k1h && r.n_layers > 0 && !r.sw.ffn_fp32;
    if (h8 && gat_rows_lds_bytes(r.n) > kModelLdsPerCU) return refuse(GNNGLS_ERR_UNSUPPORTED, FWD_K1_LDS, (int64_t)gat_rows_lds_bytes(r.n));
    if (beyond_k1h) return refuse(GNNGLS_ERR_UNSUPPORTED, FWD_K1H_NODES, kMaxNodes);
    const int64_t image_need = (int64_t)prepared_bytes(r.n_layers);
    if (!r.one_call && r.image_given && r.image_bytes < image_need) return refuse(GNNGLS_ERR_ARG, FWD_IMAGE_SMALL, image_need);
    // no image keeps the feed-forward block on the fp32 matrix pipe (as GNNGLS_FFN_FP32=1 does: A/B runs)
    const bool prep = p.use_image = (r.one_call ? p.build_image : r.image_given) && !r.sw.ffn_fp32;
    const long N = (long)r.n * (r.n - 1) / 2;
    const int64_t per_instance = (int64_t)forward_layout(N, r.n_heads).end;
    p.Bc = r.workspace_avail / per_instance;
    if (p.Bc < 1) { p.Bc = 0; return refuse(GNNGLS_ERR_ARG, FWD_WORKSPACE_SMALL, per_instance + 256); }
    if (p.Bc > r.B) p.Bc = r.B;
    p.ws = forward_layout(p.Bc * N, r.n_heads);

    // models.py:66; with an image also ft = fc(h) of layer 0 (models.py:23), both straight from the input features
    const bool fused_fc0 = prep && r.n_layers > 0 && r.in_dim <= kEmbedFcMaxIn;
    // one input feature: the first GATConv runs in its rank-1 form and no ft is written (the image holds 8-head coefficients)
    const bool rank1 = fused_fc0 && r.in_dim == 1 && r.n <= kRank1MaxNodes && r.sw.rank1_mode != 0 && h8;
    // ... and then the first feed-forward launch forms its input from the one feature and the compact partials: no embedding
    // pass at all, neither h_0 nor ft_0 nor 128-wide partials of the first layer in memory (rank1_mode 2: keep them, A/B runs)
    const bool compact = rank1 && r.sw.rank1_mode != 2;
    p.embed = compact ? EMBED_NONE : rank1 ? EMBED_FC_H_ONLY : fused_fc0 ? EMBED_FC : EMBED_PLAIN;
    const AttnStep attn = h8 ? gat_rows_step(r.n, r.sw.gat_heads) : gat_heads_rows_step(r.n, r.n_heads);
    const AttnStep attn_rank1 = {compact ? ATTN_RANK1_COMPACT : ATTN_RANK1, kH, gat_rank1_waves(r.n), gat_rank1_lds_bytes(r.n), kF, false};
    auto step = [&](bool is_first, bool is_last) {
        LayerStep s;
        // ft = fc(h), models.py:23: a launch of its own for the first layer (and for every layer on the fp32 path); on the bf16x3
        // path the feed-forward launch of layer l - 1 has already written it (fc folded into that kernel's tail)
        s.fc_launch = (is_first && !fused_fc0) || !prep;
        s.attn = is_first && rank1 ? attn_rank1 : attn;
        // gat_combine + FFN1 + FFN2 in one launch; the last layer's also applies the decision layer (models.py:69)
        s.ffn = {prep, prep && !is_last, prep && is_last, is_first && compact};
        return s;
    };
    p.first = step(true, r.n_layers == 1); p.middle = step(false, false); p.last = step(false, true);
    p.decision_launch = !(prep && r.n_layers > 0);
    return p;
}

TrainLayout train_layout(long M, int n_layers, int n_heads) {
    TrainLayout w;
    size_t p = 0;
    auto take = [&p](size_t bytes) { const size_t q = p; p = (p + bytes + 255) & ~(size_t)255; return q; };
    const size_t L = (size_t)n_layers, fl = sizeof(float);
    w.M = M; w.row = (size_t)M * kD * fl; w.stat_w = n_heads == 16 ? 32 : 16;
    const size_t stats = (size_t)M * w.stat_w * fl, dlr = stats / 2, wt = (size_t)kFfnHidden * kD * fl;
    w.H = take(w.row * (L + 1)); w.FT = take(w.row * L); w.G = take(w.row * L); w.H1 = take(w.row * L); w.H3 = take(w.row * L);
    w.HID = take(4 * w.row * L); w.ATT = take(stats * L); w.BN = take(L * BN_SLOTS * kD * fl);
    w.PART = take(2 * w.row); w.PMS = take(2 * stats);
    w.DA = take(w.row); w.DB = take(w.row); w.X2 = take(w.row); w.DFT = take(w.row);
    w.DL = take(2 * dlr); w.DR = w.DL + dlr;
    w.W2T = take(2 * wt); w.W1T = w.W2T + wt;
    w.COEF = take((3 * kD + kD + kFfnHidden) * fl); w.ONES = w.COEF + 3 * kD * fl; w.ZEROS = w.ONES + kD * fl;
    w.CSP = take((size_t)kColsumMaxBlocks * 2 * kFfnHidden * sizeof(double));
    w.TNP = take((size_t)gemm_tn_chunks(M) * (kD * kFfnHidden + kFfnHidden) * fl);
    w.end = p;
    return w;
}

int64_t train_workspace_bytes(int B, int n, int n_layers, int n_heads) {
    if (!heads_supported(n_heads)) return 0;
    if (B < 1 || n < 2 || n > 65535 || n_layers < 0 || n_layers > 4096) return 0;
    return (int64_t)train_layout((long)B * ((long)n * (n - 1) / 2), n_layers, n_heads).end + 256;
}

namespace {
template <int F>
AttnBwdStep heads_bwd_step(int n) {
    using S = BwdShape<F>;
    return {ATTN_K1H, 0, F, heads_bwd_lds<F>(n), kD / S::CW, S::WAVES};
}
}  // namespace

TrainPlan train_plan(const TrainRequest &r) {
    TrainPlan p{};
    p.status = GNNGLS_OK; p.why = TRAIN_OK;
    auto refuse = [&p](int status, TrainRefusal why, int64_t number) { p.status = status; p.why = why; p.number = number; return p; };
    if (!heads_supported(r.n_heads)) return refuse(GNNGLS_ERR_UNSUPPORTED, TRAIN_BAD_HEADS, r.n_heads);
    if (!r.pointers_given || r.B < 1 || r.n < 3 || r.in_dim < 1 || r.n_layers < 0) return refuse(GNNGLS_ERR_ARG, TRAIN_BAD_ARG, 0);
    // the backward's register-resident accumulators set the limit; no LDS refusal below it (model_policy.h asserts every carve)
    if (r.n > kTrainMaxNodes) return refuse(GNNGLS_ERR_UNSUPPORTED, TRAIN_BWD_NODES, kTrainMaxNodes);
    // (as the ABI's size query answers: 0, and so no refusal here, beyond 4096 layers)
    const int64_t need = train_workspace_bytes(r.B, r.n, r.n_layers, r.n_heads);
    if (r.workspace_bytes < need) return refuse(GNNGLS_ERR_ARG, TRAIN_WORKSPACE_SMALL, need);
    p.ws = train_layout((long)r.B * ((long)r.n * (r.n - 1) / 2), r.n_layers, r.n_heads);
    p.attn = r.n_heads == 8 ? gat_rows_step(r.n, r.gat_heads) : gat_heads_rows_step(r.n, r.n_heads);
    p.combine = r.n_heads == 16 ? COMBINE_HEADS16 : COMBINE_SLOTS;
    switch (r.n_heads) {
    case 8: p.bwd = {ATTN_K1, gat_bwd_tiles(r.n), kF, gat_bwd_lds_bytes(r.n), kH / kGatBwdHeads, kGatBwdHeads}; break;
    case 1: p.bwd = heads_bwd_step<128>(r.n); break;
    case 2: p.bwd = heads_bwd_step<64>(r.n); break;
    case 4: p.bwd = heads_bwd_step<32>(r.n); break;
    default: p.bwd = heads_bwd_step<8>(r.n); break;
    }
    return p;
}

}  // namespace gnngls
