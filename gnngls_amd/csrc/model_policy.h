// model_policy.h -- what the regret model's kernels (model_kernels.hip, heads_kernels.hip, train_kernels.hip) and the plans of the
// forward and of the training step (model_plan.cpp: plain host C++) both need: the model's dimensions, the LDS carve of each
// attention kernel, forward and backward, the launch-shape rules measured on them and the grids of the training step's reductions.
// constexpr only, no HIP include; a kernel file asserts the relations it relies on.
#pragma once
#include <stddef.h>

namespace gnngls {

constexpr int kD = 128;        // embed_dim
constexpr int kH = 8;          // heads of the K1 kernels (model_kernels.hip)
constexpr int kF = 16;         // their head dim
constexpr size_t kModelLdsPerCU = 160 * 1024;        // LDS of a CU (MI355X)
constexpr int kMaxNodes = 257;                  // n limit of every kernel of heads_kernels.hip (n - 1 <= 256 sources per row)
constexpr int kEmbedFcMaxIn = 32;     // input features the fused embed + first fc is prepared for (embed_fc_kernel)
// the embed-fc image: A [in_dim,128], b' [128] and for in_dim == 1 the logit coefficients al | bl | ar | br [8] each
constexpr size_t kEmbedFcBytes = ((size_t)(kEmbedFcMaxIn + 1) * kD + 4 * kH) * sizeof(float);
constexpr int kFfnStageBytes = 8 * 3 * 64 * 16;    // one weight stage of the bf16x3 feed-forward: 8 tiles x 3 pieces x 64 lanes x 16 B
constexpr size_t kFfnPackedBytes = (size_t)(2 * 16 + 4) * kFfnStageBytes;  // W1p + W2p + the next layer's fc: 884,736 B

constexpr bool heads_supported(int n_heads) { return n_heads == 1 || n_heads == 2 || n_heads == 4 || n_heads == 8 || n_heads == 16; }
constexpr int idle_wave_slots(int units, int waves) { return (units + waves - 1) / waves * waves - units; }

// ---- K1: gat_rows_kernel<HS>, 8 heads of 16 features, HS of them per workgroup ---------------------------------------------------
constexpr size_t gat_rows_lds_bytes_hs(int n, int hs) {
    const size_t ns = (size_t)n - 1;
    return ns * (size_t)(hs * kF + 16) * 4 + 4 * ns * hs * 4 + (size_t)hs * 4 * 4 + ns * 4 + 16;
}
// heads per workgroup: all 8 while at least two such workgroups fit a CU, else the head-split form (4).  Measured per
// launch (profiles/r02_ab_gat_heads.log): TSP200 x 256 11.5 -> 8.5 ms with the split (one -> two workgroups per CU);
// TSP100 x 1024 5.33 -> 5.69 ms, TSP50 x 2048 1.73 -> 1.82 ms (two+ workgroups already hide the prologue; the split
// only adds workgroup starts), so it is used where the unsplit tile leaves a CU with a single workgroup: from n = 117.
constexpr int gat_rows_heads(int n) { return gat_rows_lds_bytes_hs(n, kH) * 2 <= kModelLdsPerCU ? kH : 4; }
constexpr size_t gat_rows_lds_bytes(int n) { return gat_rows_lds_bytes_hs(n, gat_rows_heads(n)); }
// units = (16-destination tiles) x (head quads of the workgroup), spread over 4..8 waves: the wave count with the
// fewest idle wave slots; on ties the one that brings the CU closest to 16 resident waves at the LDS-limited
// workgroup count
constexpr int gat_rows_units(int n, int hs) { return ((n - 1 + 15) / 16) * (hs / 4); }
constexpr int gat_rows_waves(int units, size_t lds) {
    const int wgs_per_cu = (int)(kModelLdsPerCU / lds) > 0 ? (int)(kModelLdsPerCU / lds) : 1;
    const int want = 16 / wgs_per_cu > 0 ? 16 / wgs_per_cu : 1;
    int waves = 4;
    for (int w = 5; w <= 8; ++w) {
        const int idle_w = idle_wave_slots(units, w), idle_b = idle_wave_slots(units, waves);
        const int dw = w > want ? w - want : want - w, db = waves > want ? waves - want : want - waves;
        if (idle_w < idle_b || (idle_w == idle_b && dw < db)) waves = w;
    }
    return waves;
}

// ---- the rank-1 first GATConv (gat_rows_rank1_kernel, one input feature): (64 destinations, 4 heads) per wavefront --------------
constexpr int gat_rank1_waves(int n) { return ((n - 1 + 63) / 64) * 2 < 4 ? 4 : ((n - 1 + 63) / 64) * 2; }
constexpr size_t gat_rank1_lds_bytes(int n) { return (size_t)(n - 1) * (2 + 2 * kH) * sizeof(float) + kH * 4 * sizeof(float) + 16; }
constexpr int kRank1MaxNodes = 255;

// ---- K1h: gat_heads_rows_kernel<F>, H = 128 / F heads of F features --------------------------------------------------------------
template <int F>
struct HeadShape {
    static constexpr int CW = F == 128 ? 128 : 64;      // columns per workgroup: a head is never split (el / er need all F)
    static constexpr int HS = CW / F;                    // heads per workgroup: 1, 1, 2, 8
    static constexpr int HG = kD / CW;                   // workgroups per (instance, row)
    static constexpr int LDF = CW + 16;                  // LDS row stride (floats) of the ft tile, 16 (mod 64) as gat_rows_kernel
    static constexpr int UH = F >= 64 ? 1 : 64 / F;      // heads of a 64-column unit: 1, 1, 2, 8
    static constexpr int UNITS = CW / 64;                // units per 16-destination tile
    static constexpr int LP = F >= 16 ? F / 16 : 1;      // lanes per (source, head) logit pair, 16 (F = 8: 8) features each
};
template <int F>
constexpr size_t heads_rows_lds(int n) {
    using S = HeadShape<F>;
    const size_t ns = (size_t)n - 1;
    return ns * S::LDF * 4 + 4 * ns * S::HS * 4 + (size_t)S::HS * 4 * 4 + ns * 4 + 16;
}
constexpr size_t gat_heads_rows_lds_bytes(int n, int n_heads) {
    return n_heads == 1 ? heads_rows_lds<128>(n) : n_heads == 2 ? heads_rows_lds<64>(n) : n_heads == 4 ? heads_rows_lds<32>(n)
                                                                                                         : heads_rows_lds<8>(n);
}
// units = (16-destination tiles) x (64-column units) over 4..8 waves: the wave count with the fewest idle wave slots (at least
// 4: the top-2 pass takes 32 lanes per head of the workgroup); no residency tie-break here
constexpr int gat_heads_rows_units(int n, int n_heads) { return ((n - 1 + 15) / 16) * (n_heads == 1 ? 2 : 1); }
constexpr int gat_heads_rows_waves(int units) {
    int waves = 4;
    for (int w = 5; w <= 8; ++w)
        if (idle_wave_slots(units, w) < idle_wave_slots(units, waves)) waves = w;
    return waves;
}

// ---- K1 backward: gat_bwd_rows_kernel<MAXT> (train_kernels.hip), 8 heads of 16 features, kGatBwdHeads of them per workgroup -------
constexpr int kGatBwdHeads = 2;                    // heads per workgroup (one wave each): the LDS tile of a workgroup covers
                                                   // 16*kGatBwdHeads columns of ft / dOut, so several workgroups share a CU
                                                   // and the staging of one overlaps the MFMA phase of the others
constexpr int kGatBwdThreads = 64 * kGatBwdHeads;
constexpr int kGatBwdMaxTiles = 16;                // 16-node source tiles per row the largest instantiation holds: n - 1 <= 256
constexpr int kGatBwdRowStride = 16 * kGatBwdHeads + 4;   // LDS row stride (floats): a ds_read_b128 of 16 consecutive rows at one
                                                   // column offset touches 16 disjoint groups of 4 banks; 4 rows 4 apart
                                                   // (MFMA B fragment) land on disjoint 16-bank groups  (36, 68, 132)
constexpr int kGatBwdMaxNodes = 16 * kGatBwdMaxTiles + 1;  // register-resident accumulators: one per 16-node source tile
constexpr size_t gat_bwd_lds_bytes(int n) {
    const size_t ns = (size_t)n - 1;
    return 2 * ns * kGatBwdRowStride * 4 + ns * kGatBwdHeads * 4 + ns * kGatBwdHeads * 16 + ns * 4 + 16;
}
// source tiles the instantiation keeps accumulators for (5 VGPRs each): the smallest of 9 (n <= 145, the reference's training
// sizes up to TSP100), 13 (n <= 209: TSP200) and 16 (n <= 257) that covers n
constexpr int gat_bwd_tiles(int n) { return (n - 1 + 15) / 16 <= 9 ? 9 : (n - 1 + 15) / 16 <= 13 ? 13 : kGatBwdMaxTiles; }

// ---- K1h backward: gat_heads_bwd_rows_kernel<F> (heads_kernels.hip) ----------------------------------------------------------------
template <int F>
struct BwdShape {
    static constexpr int CW = F == 128 ? 128 : 64;       // dOut columns staged per workgroup
    static constexpr int HB = CW / F;                    // heads per workgroup: 1, 1, 2, 8
    static constexpr int WS = HB >= 4 ? 1 : 4 / HB;      // wavefronts per head: 4, 4, 2, 1
    static constexpr int WAVES = HB * WS;                // 4, 4, 4, 8
    static constexpr int LDG = CW + 4;                   // LDS row stride (floats)
    static constexpr int KB = F >= 16 ? F / 16 : 1;      // 16-feature blocks of a head
    static constexpr int LP = F >= 16 ? F / 16 : 1;      // lanes per (slot, head) in the statistics pass
    static constexpr int ATS = F >= 16 ? 16 : 32;        // att row stride: slot layout (8 + 8) or per head (16 + 16)
};
template <int F>
constexpr size_t heads_bwd_lds(int n) {
    using S = BwdShape<F>;
    const size_t ns = (size_t)n - 1;
    return ns * S::HB * 16 + ns * S::LDG * 4 + ns * S::HB * 4 + (size_t)S::WAVES * ns * 4 + ns * 4 + 16;
}
constexpr size_t gat_heads_bwd_lds_bytes(int n, int n_heads) {
    return n_heads == 1 ? heads_bwd_lds<128>(n) : n_heads == 2 ? heads_bwd_lds<64>(n) : n_heads == 4 ? heads_bwd_lds<32>(n)
                                                                                                       : heads_bwd_lds<8>(n);
}

// ---- the training step's limit is the backward's, and there every carve (monotone in n) leaves room: no LDS refusal in the step ----
constexpr int kTrainMaxNodes = kGatBwdMaxNodes;
static_assert(kTrainMaxNodes <= kMaxNodes, "the K1h kernels (forward and backward) hold n - 1 <= 256 sources per row");
static_assert(gat_rows_lds_bytes(kTrainMaxNodes) <= kModelLdsPerCU && gat_bwd_lds_bytes(kTrainMaxNodes) <= kModelLdsPerCU,
              "8 heads: the K1 forward and backward tiles fit a CU's LDS up to the training limit");
static_assert(heads_rows_lds<128>(kTrainMaxNodes) <= kModelLdsPerCU && heads_rows_lds<64>(kTrainMaxNodes) <= kModelLdsPerCU &&
              heads_rows_lds<32>(kTrainMaxNodes) <= kModelLdsPerCU && heads_rows_lds<8>(kTrainMaxNodes) <= kModelLdsPerCU,
              "1, 2, 4, 16 heads: the K1h forward tile fits a CU's LDS up to the training limit");
static_assert(heads_bwd_lds<128>(kTrainMaxNodes) <= kModelLdsPerCU && heads_bwd_lds<64>(kTrainMaxNodes) <= kModelLdsPerCU &&
              heads_bwd_lds<32>(kTrainMaxNodes) <= kModelLdsPerCU && heads_bwd_lds<8>(kTrainMaxNodes) <= kModelLdsPerCU,
              "1, 2, 4, 16 heads: the K1h backward tile fits a CU's LDS up to the training limit");

// ---- grids of the training step's reductions (train_kernels.hip); the workspace holds their partials -----------------------------
constexpr int kColsumMaxBlocks = 512;     // partial buffer: kColsumMaxBlocks * 2 * 512 doubles
constexpr int kGemmTnMaxChunks = 256;     // partial buffer: kGemmTnMaxChunks * (128 * 512 + 512) floats
constexpr int colsum_blocks(long M, int C) {            // 16 rows per row lane of a block, 1024 / C row lanes
    const long rows = 1024 / C * 16, want = (M + rows - 1) / rows;
    return (int)(want > kColsumMaxBlocks ? kColsumMaxBlocks : want < 1 ? 1 : want);
}
constexpr int gemm_tn_chunks(long M) {                  // >= 128 rows (4 k-tiles) per chunk, at most kGemmTnMaxChunks chunks
    const long want = (M + 127) / 128;
    return (int)(want > kGemmTnMaxChunks ? kGemmTnMaxChunks : want < 1 ? 1 : want);
}

}  // namespace gnngls
