// forward_plan_sweep.cpp -- stand-alone sweep of the regret forward's plan (csrc/model_plan.cpp, linked alone: no HIP).
//
//   forward_plan_sweep GRID > records
//
// GRID (written by test_forward_plan_cpu.py from the fixture) holds one line of integers per grid point:
//   n n_heads n_layers in_dim form B workspace_avail image_bytes packed_floats
// (form 0 one-call, 1 prepared image, 2 prepared NULL).  Every point is planned under the four switch settings of the fixture
// (default, fp32 feed-forward, rank-1 mode 0, rank-1 mode 2; setting-major order) and checked for consistency; per point and
// setting eight int32 go to stdout: the status, Bc, and the profile spans per kind that the plan's steps imply, summed over chunks
// and layers (embed, gemm_fc, gat_rows, gat_rows_rank1, ffn_fused, decision).
// The test builds this with -fsanitize=address,undefined, so a plan that reads out of range or overflows ends the run.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../gnngls_amd/csrc/model_plan.h"

using namespace gnngls;

static void require(bool ok, const char *what, const ForwardRequest &r) {
    if (ok) return;
    fprintf(stderr, "forward_plan_sweep: %s at n=%d B=%d in_dim=%d layers=%d heads=%d one_call=%d image=%d avail=%lld switches=(%d,%d,%d)\n",
            what, r.n, r.B, r.in_dim, r.n_layers, r.n_heads, (int)r.one_call, (int)r.image_given, (long long)r.workspace_avail,
            (int)r.sw.ffn_fp32, r.sw.rank1_mode, r.sw.gat_heads);
    exit(1);
}

static void point(const ForwardRequest &r, long packed_floats, std::vector<int32_t> &out) {
    const ForwardPlan p = forward_plan(r);
    int32_t rec[8] = {p.status, (int32_t)p.Bc, 0, 0, 0, 0, 0, 0};
    require(packed_model(r.in_dim, r.n_layers).total == packed_floats, "packed_model().total", r);
    require((p.status == 0) == (p.why == FWD_OK), "status and refusal disagree", r);
    if (p.status == 0) {
        const long N = (long)r.n * (r.n - 1) / 2, M = p.Bc * N;
        const size_t row = (size_t)M * 128 * 4, per_node = forward_layout(1, r.n_heads).end;
        const ForwardLayout &w = p.ws;
        require(p.Bc >= 1 && p.Bc <= r.B, "Bc", r);
        // the regions are disjoint, lie in order and end within the given bytes
        require(w.h == 0 && w.ft >= w.h + row && w.part >= w.ft + row && w.part_ms >= w.part + 2 * row &&
                w.h2 >= w.part_ms + (size_t)2 * M * 16 * 4 && w.hms >= w.h2 + row &&
                w.end >= w.hms + (r.n_heads == 16 ? (size_t)2 * M * 32 * 4 : 0), "workspace regions overlap", r);
        require((int64_t)w.end <= r.workspace_avail, "workspace regions end beyond the given bytes", r);
        require(w.end == (size_t)M * per_node && (int64_t)((size_t)p.Bc * N * per_node) <= r.workspace_avail, "Bc * N * bytes_per_node", r);
        require(p.use_image == ((r.one_call ? p.build_image : r.image_given) && !r.sw.ffn_fp32), "use_image", r);
        const int chunks = (int)((r.B + p.Bc - 1) / p.Bc);
        rec[2] = p.embed != EMBED_NONE ? chunks : 0;
        for (int l = 0; l < r.n_layers; ++l) {
            const LayerStep &s = p.layer(l);
            const AttnStep &a = s.attn;
            const bool rank1 = a.form == ATTN_RANK1 || a.form == ATTN_RANK1_COMPACT;
            require(a.waves >= 4 && a.waves <= 8 && a.lds > 0 && a.lds <= kModelLdsPerCU, "attention launch shape", r);
            require(!rank1 || (l == 0 && r.in_dim == 1 && r.n_heads == 8 && p.use_image), "rank-1 attention out of place", r);
            require((a.form == ATTN_K1H) == (r.n_heads != 8) && a.merge16 == (a.form == ATTN_K1H && r.n_heads == 16), "attention form", r);
            require(a.form != ATTN_K1 || ((a.heads_per_wg == 8 || a.heads_per_wg == 4) && a.lds == gat_rows_lds_bytes_hs(r.n, a.heads_per_wg)), "K1 shape", r);
            require(a.form != ATTN_K1H || (a.F * r.n_heads == 128 && a.lds == gat_heads_rows_lds_bytes(r.n, r.n_heads)), "K1h shape", r);
            require(s.ffn.bf16x3 == p.use_image && (s.ffn.bf16x3 || !(s.ffn.writes_next_ft || s.ffn.decision || s.ffn.rank1_input)), "ffn form", r);
            require(s.ffn.decision == (p.use_image && l + 1 == r.n_layers) && s.ffn.writes_next_ft == (p.use_image && l + 1 < r.n_layers), "ffn tail", r);
            require(s.ffn.rank1_input == (a.form == ATTN_RANK1_COMPACT) && (a.form != ATTN_RANK1_COMPACT || p.embed == EMBED_NONE), "rank-1 input", r);
            // ft of layer l exists before its attention reads it: from the embedding pass, the previous feed-forward, or fc
            require(rank1 || s.fc_launch || (l == 0 ? p.embed == EMBED_FC : p.layer(l - 1).ffn.writes_next_ft), "nobody writes ft", r);
            rec[3] += s.fc_launch ? chunks : 0;
            rec[rank1 ? 5 : 4] += chunks;
            rec[6] += chunks;
        }
        require(p.decision_launch == !(r.n_layers > 0 && p.layer(r.n_layers - 1).ffn.decision), "decision layer", r);
        require(p.embed != EMBED_NONE || (r.n_layers > 0 && p.first.ffn.rank1_input), "no embedding", r);
        rec[7] = p.decision_launch ? chunks : 0;
    } else {
        require(p.Bc == 0, "a refused plan with chunks", r);
    }
    require(!p.build_image || (r.one_call && r.n_layers > 0 && !r.sw.ffn_fp32), "build_image", r);
    out.insert(out.end(), rec, rec + 8);
}

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: forward_plan_sweep GRID\n"); return 2; }
    FILE *f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    struct Row { int n, H, L, d, form, B; long long avail, image, packed; };
    std::vector<Row> rows;
    Row q;
    while (fscanf(f, "%d %d %d %d %d %d %lld %lld %lld", &q.n, &q.H, &q.L, &q.d, &q.form, &q.B, &q.avail, &q.image, &q.packed) == 9)
        rows.push_back(q);
    fclose(f);
    if (rows.empty()) { fprintf(stderr, "forward_plan_sweep: bad grid file\n"); return 2; }
    const ForwardSwitches settings[4] = {{false, -1, 0}, {true, -1, 0}, {false, 0, 0}, {false, 2, 0}};
    std::vector<int32_t> out;
    for (const ForwardSwitches &sw : settings)
        for (const Row &g : rows) {
            ForwardRequest r{};
            r.n = g.n; r.B = g.B; r.in_dim = g.d; r.n_layers = g.L; r.n_heads = g.H; r.pointers_given = true;
            r.one_call = g.form == 0; r.image_given = g.form == 1; r.image_bytes = g.form == 1 ? g.image : 0;
            r.workspace_avail = g.avail; r.sw = sw;
            point(r, (long)g.packed, out);
        }
    return fwrite(out.data(), sizeof(int32_t), out.size(), stdout) == out.size() ? 0 : 1;
}
