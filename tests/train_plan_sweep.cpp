// train_plan_sweep.cpp -- stand-alone sweep of the training step's plan and workspace layout (csrc/model_plan.cpp, linked alone: no HIP).
//
//   train_plan_sweep GRID > records
//
// GRID (written by test_train_plan_cpu.py from the fixture's size axes and recorded refusals) holds one line of integers per request:
//   n B in_dim n_layers n_heads pointers_given workspace_mode gat_heads
// (workspace_mode 0: the bytes the size query names, 1: one byte less, 2: zero).  Per request four int64 go to stdout: what
// gnngls_regret_train_workspace_bytes_heads answers (train_workspace_bytes), train_layout(...).end + 256 where a layout exists
// (B >= 1, 2 <= n <= 65535, n_layers >= 0, a supported head count; else 0), the plan's status and its refusal reason.  Wherever a layout
// exists it is checked region by region against sizes worked out here, and every accepted plan against the policy's rules.
// The test builds this with -fsanitize=address,undefined, so a plan that reads out of range or overflows ends the run.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../gnngls_amd/csrc/model_plan.h"

using namespace gnngls;

struct Row { int n, B, d, L, H, ptrs, ws_mode, gat_heads; };

static void require(bool ok, const char *what, const Row &g) {
    if (ok) return;
    fprintf(stderr, "train_plan_sweep: %s at n=%d B=%d in_dim=%d layers=%d heads=%d pointers=%d workspace_mode=%d gat_heads=%d\n", what,
            g.n, g.B, g.d, g.L, g.H, g.ptrs, g.ws_mode, g.gat_heads);
    exit(1);
}

static size_t up256(size_t v) { return (v + 255) / 256 * 256; }

// regions ascending, 256-byte aligned, each exactly as large as its contents rounded up; the named parts inside them
static void check_layout(const TrainLayout &w, long M, int L, int H, const Row &g) {
    const size_t row = (size_t)M * 128 * 4, sw = H == 16 ? 32 : 16, stats = (size_t)M * sw * 4;
    const long want_chunks = (M + 127) / 128 > 256 ? 256 : (M + 127) / 128 < 1 ? 1 : (M + 127) / 128;
    require(gemm_tn_chunks(M) == want_chunks, "gemm_tn_chunks", g);
    const size_t at[] = {w.H, w.FT, w.G, w.H1, w.H3, w.HID, w.ATT, w.BN, w.PART, w.PMS, w.DA, w.DB, w.X2, w.DFT, w.DL, w.W2T, w.COEF, w.CSP,
                         w.TNP, w.end};
    const size_t size[] = {row * (L + 1), row * L, row * L, row * L, row * L, 4 * row * L, stats * L, (size_t)L * 8 * 128 * 4, 2 * row,
                           2 * stats, row, row, row, row, stats, (size_t)2 * 512 * 128 * 4, (size_t)(3 * 128 + 128 + 512) * 4,
                           (size_t)kColsumMaxBlocks * 2 * 512 * 8, (size_t)want_chunks * (128 * 512 + 512) * 4};
    static_assert(sizeof(at) / sizeof(at[0]) == sizeof(size) / sizeof(size[0]) + 1, "a size per region");
    require(at[0] == 0, "the first region starts at the base", g);
    for (size_t i = 0; i + 1 < sizeof(at) / sizeof(at[0]); ++i) {
        require(at[i] % 256 == 0, "a region is not 256-byte aligned", g);
        require(at[i + 1] == up256(at[i] + size[i]), "a region overlaps the next or leaves a gap", g);
    }
    require(w.end % 256 == 0 && w.M == M && w.row == row && w.stat_w == (int)sw, "M, row, stat_w", g);
    // PMS / ATT / DLR hold 16 floats per row (d el, d er: 8 each), exactly twice that with 16 heads
    const TrainLayout w8 = train_layout(M, L, 8);
    const size_t k = H == 16 ? 2 : 1;
    require(w.DA - w.PMS == up256(k * 2 * (size_t)M * 16 * 4), "PMS width", g);
    require(w.BN - w.ATT == up256(k * (size_t)M * 16 * 4 * L) && w.att(1) - w.att(0) == k * (w8.att(1) - w8.att(0)), "ATT width", g);
    require(w.W2T - w.DL == up256(k * 2 * (size_t)M * 8 * 4) && w.DR - w.DL == k * (size_t)M * 8 * 4 && w.DR - w.DL == k * (w8.DR - w8.DL),
            "DLR width", g);
    require(w.W1T == w.W2T + (size_t)512 * 128 * 4, "the transposed weights", g);
    require(w.ONES == w.COEF + 3 * 128 * 4 && w.ZEROS == w.ONES + 128 * 4 && w.ZEROS + 512 * 4 <= w.CSP, "the coefficient block", g);
    require(w.h(0) == w.H && w.h(L) + row == w.H + size[0] && w.ft(L) == w.FT + size[1] && w.g(L) == w.G + size[2] &&
            w.h1(L) == w.H1 + size[3] && w.h3(L) == w.H3 + size[4] && w.hid(L) == w.HID + size[5] && w.att(L) == w.ATT + size[6],
            "the per-layer strides of the saved tensors", g);
    require(w.bn(0, BN_MEAN1) == w.BN && w.bn(L, BN_MEAN1) == w.BN + size[7] && w.bn(0, BN_SHIFT2) - w.bn(0, BN_MEAN1) == 7 * 128 * 4 &&
            w.bn(0, BN_INVSTD1) - w.bn(0, BN_MEAN1) == 128 * 4, "the BatchNorm slots", g);
    require(batch_stat(0, STAT_MEAN1) == 0 && batch_stat(0, STAT_VAR2) == 3 * 128 && batch_stat(1, STAT_MEAN1) == 4 * 128, "bn_batch_stats slots", g);
}

static void check_plan(const TrainPlan &p, const TrainRequest &r, const Row &g) {
    const AttnStep want = r.n_heads == 8 ? gat_rows_step(r.n, r.gat_heads) : gat_heads_rows_step(r.n, r.n_heads);
    const AttnStep &a = p.attn;
    require(a.form == want.form && a.heads_per_wg == want.heads_per_wg && a.waves == want.waves && a.lds == want.lds && a.F == want.F &&
            a.merge16 == want.merge16, "the forward attention is not the inference forward's", g);
    require((a.form == ATTN_K1) == (r.n_heads == 8) && (r.gat_heads != 0 || a.lds <= kModelLdsPerCU), "forward attention form", g);
    require((p.combine == COMBINE_HEADS16) == (r.n_heads == 16) && a.merge16 == (p.combine == COMBINE_HEADS16), "combine form", g);
    const AttnBwdStep &b = p.bwd;
    const int nt = (r.n - 1 + 15) / 16;
    require((b.form == ATTN_K1) == (r.n_heads == 8) && b.lds > 0 && b.lds <= kModelLdsPerCU && b.waves * 64 <= 512, "attention backward shape", g);
    if (b.form == ATTN_K1) {
        require(b.tiles == (nt <= 9 ? 9 : nt <= 13 ? 13 : 16) && b.tiles >= nt && b.lds == gat_bwd_lds_bytes(r.n) && b.F == 16 &&
                b.wgs_per_row * b.waves == 8, "K1 backward", g);
    } else {
        require(b.F * r.n_heads == 128 && b.lds == gat_heads_bwd_lds_bytes(r.n, r.n_heads) && b.wgs_per_row == (r.n_heads == 1 ? 1 : 2) &&
                b.waves == (r.n_heads == 16 ? 8 : 4), "K1h backward", g);
    }
}

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: train_plan_sweep GRID\n"); return 2; }
    FILE *f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    std::vector<Row> rows;
    Row q;
    while (fscanf(f, "%d %d %d %d %d %d %d %d", &q.n, &q.B, &q.d, &q.L, &q.H, &q.ptrs, &q.ws_mode, &q.gat_heads) == 8) rows.push_back(q);
    fclose(f);
    if (rows.empty()) { fprintf(stderr, "train_plan_sweep: bad grid file\n"); return 2; }
    std::vector<int64_t> out;
    for (const Row &g : rows) {
        const int64_t bytes = train_workspace_bytes(g.B, g.n, g.L, g.H);
        const long M = (long)g.B * ((long)g.n * (g.n - 1) / 2);
        int64_t layout_bytes = 0;
        if (g.B >= 1 && g.n >= 2 && g.n <= 65535 && g.L >= 0 && heads_supported(g.H)) {
            const TrainLayout w = train_layout(M, g.L, g.H);
            check_layout(w, M, g.L, g.H, g);
            layout_bytes = (int64_t)w.end + 256;
        }
        TrainRequest r{};
        r.n = g.n; r.B = g.B; r.in_dim = g.d; r.n_layers = g.L; r.n_heads = g.H; r.pointers_given = g.ptrs != 0;
        r.workspace_bytes = g.ws_mode == 0 ? bytes : g.ws_mode == 1 ? bytes - 1 : 0; r.gat_heads = g.gat_heads;
        const TrainPlan p = train_plan(r);
        require((p.status == 0) == (p.why == TRAIN_OK), "status and refusal disagree", g);
        if (p.status == 0) {
            require((int64_t)p.ws.end + 256 == bytes && bytes == layout_bytes && p.ws.M == M, "the plan's layout is not the size query's", g);
            check_plan(p, r, g);
        } else {
            require(p.why != TRAIN_WORKSPACE_SMALL || (p.number == bytes && bytes > r.workspace_bytes), "the bytes a refusal names", g);
            require(p.why != TRAIN_BWD_NODES || (p.number == 257 && g.n > 257), "the limit a refusal names", g);
        }
        const int64_t rec[4] = {bytes, layout_bytes, p.status, (int64_t)p.why};
        out.insert(out.end(), rec, rec + 4);
    }
    return fwrite(out.data(), sizeof(int64_t), out.size(), stdout) == out.size() ? 0 : 1;
}
