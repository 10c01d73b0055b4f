// gls_plan_sweep.cpp -- stand-alone sweep of the search kernel's launch plan (csrc/gls_plan.cpp, linked alone: no HIP).
//
//   gls_plan_sweep GRID > records
//
// GRID (written by test_gls_plan_cpu.py from the fixture) holds five lines of integers: n values, B values, penalty_bits
// values, the n values of the override grid, and the override configs as (team mode, prune mode, thread override) triples.
// For every point -- the default overrides over the first n list, then each config over the second -- and both values of
// first_improvement, the plan is made four times (want_trace x want_count) and checked for consistency; the seven fields
// gnngls_gls_describe_run reports go to stdout as int32 records: store code, threads, lds, per_cu, wps, team, edge_form.
// The test builds this with -fsanitize=address,undefined, so a plan that reads out of range or overflows ends the run.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <sstream>
#include <string>
#include <vector>

#include "../gnngls_amd/csrc/gls_plan.h"

using gnngls::GlsPlan;
using gnngls::GlsRequest;

static void require(bool ok, const char *what, const GlsRequest &r) {
    if (ok) return;
    fprintf(stderr, "gls_plan_sweep: %s at n=%d B=%d bits=%d fi=%d trace=%d count=%d overrides=(%d,%d,%d)\n", what, r.n, r.B,
            r.penalty_bits, (int)r.first_improvement, (int)r.want_trace, (int)r.want_count, r.team_mode, r.prune_mode, r.threads_override);
    exit(1);
}

static void point(GlsRequest r, std::vector<int32_t> &out) {
    GlsPlan base{};
    for (int v = 0; v < 4; ++v) {
        r.want_trace = v & 1; r.want_count = v & 2;
        const GlsPlan p = gnngls::gls_plan(r);
        if (v == 0) base = p;
        // what a caller asks to have recorded never moves the launch shape
        require(p.store == base.store && p.penalty_bits == base.penalty_bits && p.threads == base.threads && p.lds == base.lds &&
                p.per_cu == base.per_cu && p.wps == base.wps && p.team == base.team && p.prune == base.prune && p.gp == base.gp &&
                p.edge_form == base.edge_form && p.first_improvement == r.first_improvement, "plan depends on want_trace / want_count", r);
        require(p.trace == r.want_trace, "trace", r);
        require(!(p.count && p.count_unknown) && (p.count || p.count_unknown) == (r.want_count && p.prune), "count / count_unknown", r);
        require(!p.count || (!p.trace && p.gp >= 2 && p.store == gnngls::GLS_STORE_COMPACT && p.wps == 4), "count without a counting build", r);
        require(p.gp == 1 || p.gp == 2 || p.gp == 4, "gp", r);
        require(p.threads >= 64 && p.threads <= 1024 && p.threads % 64 == 0, "threads", r);
        require(!p.prune || (r.n >= 80 && r.n <= 255 && !r.first_improvement && p.store != gnngls::GLS_STORE_GLOBAL), "prune", r);
        require(!(p.team && p.edge_form), "team and edge form", r);
        require(p.lds == gnngls::gls_lds_bytes(r.n, p.store, p.penalty_bits, p.team), "lds", r);
    }
    const int32_t rec[7] = {base.store * 100 + (base.store == gnngls::GLS_STORE_TRI ? base.penalty_bits : 0), base.threads,
                            (int32_t)(base.lds > 0x7fffffff ? 0x7fffffff : base.lds), base.store == gnngls::GLS_STORE_GLOBAL ? 0 : base.per_cu,
                            base.wps, base.team, base.edge_form};
    out.insert(out.end(), rec, rec + 7);
}

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: gls_plan_sweep GRID\n"); return 2; }
    FILE *f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    std::vector<std::vector<int>> lines;
    char buf[1 << 16];
    while (fgets(buf, sizeof(buf), f)) {
        std::istringstream in{std::string(buf)};
        std::vector<int> row;
        for (int v; in >> v;) row.push_back(v);
        lines.push_back(row);
    }
    fclose(f);
    if (lines.size() != 5 || lines[4].size() % 3 != 0) { fprintf(stderr, "gls_plan_sweep: bad grid file\n"); return 2; }
    std::vector<int32_t> out;
    auto sweep = [&](const std::vector<int> &ns, int team, int prune, int threads) {
        for (int n : ns)
            for (int B : lines[1])
                for (int bits : lines[2])
                    for (int fi = 0; fi < 2; ++fi) {
                        GlsRequest r{};
                        r.n = n; r.B = B; r.penalty_bits = bits; r.first_improvement = fi != 0; r.num_cus = 256;
                        r.team_mode = team; r.prune_mode = prune; r.threads_override = threads;
                        point(r, out);
                    }
    };
    sweep(lines[0], -1, -1, 0);
    for (size_t c = 0; c < lines[4].size(); c += 3) sweep(lines[3], lines[4][c], lines[4][c + 1], lines[4][c + 2]);
    return fwrite(out.data(), sizeof(int32_t), out.size(), stdout) == out.size() ? 0 : 1;
}
