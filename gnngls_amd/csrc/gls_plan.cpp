// gls_plan.cpp -- the launch policy of the persistent search kernel (see gls_plan.h).  Plain C++: no HIP call, no global state.
#include "gls_plan.h"

namespace gnngls {

size_t gls_lds_bytes(int n, int store, int penalty_bits, bool team) {
    auto r16 = [](size_t x) { return (x + 15) & ~size_t(15); };
    const size_t tour_elem = store == GLS_STORE_COMPACT ? 1 : 4;
    size_t off = r16(kCtlBytes) + r16((size_t)(n + 2) * 8) + 3 * r16((size_t)(n + 1) * tour_elem);
    if (team) off += r16(kTeamCtlBytes);
    if (store == GLS_STORE_GLOBAL) off += r16((size_t)(n + 2) * 8);
    size_t ntri = (size_t)n * (n - 1) / 2;
    if (store != GLS_STORE_GLOBAL) off += r16(ntri * 8);
    if (store == GLS_STORE_TRI) off += r16(ntri * (size_t)(penalty_bits / 8));
    return off;
}

int gls_block_threads(int n, int store, int penalty_bits, bool half_scans, int forced) {
    if (forced > 0) return forced;
    if (n <= 24) return 64;
    // n <= 33 on the stores that have the half-wave descent scans: ONE wavefront using both its 32-lane halves beats two
    // wavefronts sharing the lean scans (outer iterations in 2 s, x 1000, noise guide: n = 26 24.2k -> 25.7k, n = 30 22.6k ->
    // 24.1k, n = 33 21.1k -> 22.4k)
    // (half_scans = false: the caller knows the launch ends up on an instantiation without them -- first improvement, or the
    // 64- / 80-VGPR builds -- where one wavefront would run the two-wavefront scans alone)
    if (GLS_HALF_SCANS && half_scans && n <= kHalfScanMaxNodes && penalty_bits == 32 && (store == GLS_STORE_COMPACT || store == GLS_STORE_TRI))
        return 64;
    if (n <= 48) return 128;
    if (n <= 80) return 256;
    // compact store with the lean descent scans (n <= 127), four workgroups per CU, measured at TSP100 x 1024 (outer
    // iterations per instance in 2 s, weight / noise guide): 8 waves at 64 VGPRs (108 B of scratch) 11.6k / 7.0k;
    // 4 waves at 128 VGPRs (no scratch) 12.3k / 7.5k  <- used.  (One workgroup alone on a CU prefers 8 waves, 16.1k vs
    // 14.8k, but such small batches run on the LDS-penalty store anyway.)
    if (store == GLS_STORE_COMPACT && n <= 2 * kWave - 1) return 256;
    // compact store with ONE workgroup per CU (distance triangle > 80 KB, n >= 144; TSP200): the descent is latency-bound
    // at two waves per SIMD -- 16 waves share the scans (measured TSP200 x 256, noise guide, iterations in 2 s: 8 waves
    // 4.7k, 16 waves see profiles/)
    if (store == GLS_STORE_COMPACT && 2 * gls_lds_bytes(n, GLS_STORE_COMPACT, 32) > kLdsPerCU) return 1024;
    return 512;
}

namespace {

int min_of(int a, int b) { return a < b ? a : b; }

// resident wavefronts per SIMD (= register budget) of the kernel instantiation for this configuration
int waves_per_simd(int store, int batch, int num_cus, int threads, size_t lds) {
    if (store == GLS_STORE_GLOBAL) return kGlobalWavesPerSimd;
    const int waves = threads / kWave;
    const int by_lds = (int)(kLdsPerCU / lds);
    const int per_cu4 = min_of(by_lds, 16 / waves);
    if (store == GLS_STORE_TRI) {
        // LDS-penalty store: the 128-VGPR build (no scratch) while it keeps the batch resident, else the 80-VGPR one
        // ... and only where the smaller register budget actually buys residency (n = 150: one workgroup per CU by LDS
        // either way -- the 80-VGPR build spills for nothing)
        const int per_cu6 = min_of(by_lds, 24 / waves);
        if (batch > 0 && per_cu4 >= 1 && ((long)per_cu4 * num_cus >= batch || per_cu6 <= per_cu4)) return 4;
        return kTriWavesPerSimd;
    }
    // compact store: the 128-VGPR build unless the batch only fits with 8 waves per SIMD
    return (batch > 0 && (long)per_cu4 * num_cus < batch && 32 / waves > per_cu4 && by_lds > per_cu4) ? 8 : 4;
}

// Storage configuration of the persistent search kernel for instances of n nodes: the one with the
// most resident workgroups per CU wins; ties go to the faster store (LDS penalties, 32-bit first).
void pick_store(const GlsRequest &r, GlsPlan &pick) {
    const int n = r.n, batch = r.B, cus = r.num_cus;
    pick.store = GLS_STORE_GLOBAL; pick.penalty_bits = 32; pick.per_cu = 0; pick.wps = kGlobalWavesPerSimd;
    pick.threads = gls_block_threads(n, GLS_STORE_GLOBAL, 32, true, r.threads_override);
    pick.lds = gls_lds_bytes(n, GLS_STORE_GLOBAL, 32);
    bool have = false, done = false;
    // candidates are visited fastest store first (LDS penalties 32-bit, LDS penalties 16-bit, compact); the first one
    // that keeps the whole batch resident wins, otherwise the one with the most resident workgroups per CU
    auto consider = [&](int store, int bits) {
        if (done) return;
        const size_t lds = gls_lds_bytes(n, store, bits);
        if (lds > kLdsPerCU) return;
        const int by_lds = (int)(kLdsPerCU / lds);
        // single-wavefront workgroups for n <= 33 only where the half-wave descent scans exist: best improvement, 128-VGPR build
        int threads = gls_block_threads(n, store, bits, !r.first_improvement, r.threads_override);
        // compact store, batch larger than the 128-VGPR build keeps resident at the default workgroup size: halve the
        // workgroup (down to the wavefronts the lean scans need, one per block of 64 rows) before falling back to the
        // 64-VGPR build -- TSP50 x 2048 on 2-wave workgroups at 128 VGPRs: 6.2k outer iterations per second vs 5.6k on
        // 4-wave workgroups at 64 VGPRs (profiles/r02_ab_small_n_threads.log)
        if (store == GLS_STORE_COMPACT && batch > 0) {
            const int min_threads = 64 * ((n - 1 + 63) / 64);
            while (threads > min_threads && threads > 64) {
                const int per4 = min_of(by_lds, 16 / (threads / 64));
                if ((long)per4 * cus >= batch || per4 == by_lds) break;
                threads /= 2;
            }
        }
        // wave slots per CU at the register budget of the kernel instantiation: LDS-penalty stores 80 VGPRs -> 6 waves
        // per SIMD (24 per CU); compact store 128 VGPRs -> 4 per SIMD, or its 64-VGPR build -> 8 per SIMD when only that
        // keeps the batch resident (and, without a batch size, for the capacity query)
        int wps = waves_per_simd(store, batch, cus, threads, lds);
        if (store == GLS_STORE_COMPACT && batch <= 0) wps = 8;
        if (store == GLS_STORE_TRI && bits == 16) wps = 6;            // the uint16 variant only exists as the 80-VGPR build
        // (n = 25..33 beyond the 128-VGPR residency end up on the 64-VGPR build, which has no half-wave scans, still as ONE
        // wavefront per instance: measured TSP30 x 8192, 1 s -- 64 threads keep all 8192 resident, 6.2k iterations each;
        // 128 threads halve the residency: 8.8k iterations each in two rounds of 1 s, half the aggregate rate
        // (profiles/r04_ab_threads_tsp30x8192.log))
        // batches of at most two single-wavefront workgroups per SIMD: the 256-VGPR build of the one-slot kernel
        // (not while the test hook forces the team form, which only exists on the 128-VGPR build)
        // 256-VGPR instantiation (two waves per SIMD) of the one-slot kernel: single-wavefront workgroups, n = 8 .. 33, best improvement
        const bool wps2_exists = GLS_WPS2 && GLS_HALF_SCANS && !r.first_improvement && threads == kWave && n >= kHalfScanMinNodes &&
                                 n <= kHalfScanMaxNodes && bits == 32;
        if (wps == 4 && batch > 0 && r.team_mode != 1 && wps2_exists) {
            const int per2 = min_of(by_lds, 8);
            if ((long)per2 * cus >= batch) wps = 2;
        }
        const int by_waves = (wps * 4) / (threads / 64);
        const int per_cu = min_of(by_lds, by_waves);
        const bool fits = batch > 0 && (long)per_cu * cus >= batch;
        if (!have || per_cu > pick.per_cu || fits) {
            pick.store = store; pick.penalty_bits = bits; pick.threads = threads; pick.lds = lds; pick.per_cu = per_cu; pick.wps = wps;
            have = true; done = fits;
        }
    };
    if (r.penalty_bits == -2) {               // forced compact store (falls through to the global store if it cannot fit)
        if (n <= 255) consider(GLS_STORE_COMPACT, 32);
        return;
    }
    if (r.penalty_bits < 0) return;           // forced global-memory store (exact index order, asymmetric D allowed)
    if (r.penalty_bits == 0 || r.penalty_bits == 32) consider(GLS_STORE_TRI, 32);
    // 16-bit LDS counters only on request: they overflow within a 10 s run when an uninformative guide
    // concentrates the penalties on a few edges, and an overflow costs a whole rerun of that instance
    if (r.penalty_bits == 16) consider(GLS_STORE_TRI, 16);
    if (r.penalty_bits == 0 && n <= 255) consider(GLS_STORE_COMPACT, 32);
}

int guide_passes(const GlsPlan &p, int n) {
    if (p.wps == 2) return 1;       // single-wavefront workgroups on the 256-VGPR build
    // small instances on single-wavefront workgroups (TSP20): the one-slot instantiation, whose descent scans use both
    // 32-lane halves of the wavefront (scan_*_a2a_lean_half) -- an instantiation of its own so that the register
    // allocation of the others (the TSP100 headline runs on GP = 2) does not see that code
    if (!p.first_improvement && !p.team && p.wps == 4 && p.store != GLS_STORE_GLOBAL && p.penalty_bits == 32) {
        if (GLS_HALF_SCANS && n >= kHalfScanMinNodes && n <= kHalfScanMaxNodes && p.threads == kWave) return 1;
        // the edge form of the serial perturbation phase evaluates every register slot of a lane: n <= 63 (tour positions
        // 0 .. n in one slot) runs on the one-slot instantiation whatever the workgroup shape (TSP50)
        if (GLS_EDGE_PERTURB && n <= kWave - 1) return 1;
    }
    // register-cached guide/penalty values of the tour edges: 2 passes of 64 lanes cover positions 0..n for n <= 127
    return n + 1 <= 2 * kWave ? 2 : kGuidePassesMax;
}

}  // namespace

GlsPlan gls_plan(const GlsRequest &r) {
    GlsPlan p{};
    const int n = r.n;
    p.first_improvement = r.first_improvement;
    p.trace = r.want_trace;
    pick_store(r, p);
    // + the form of the perturbation phase: on all wavefronts of the workgroup (team) when every workgroup of the batch gets a
    // CU of its own (B <= number of CUs) and is a 16-wave workgroup (TSP200 x 256: one per CU by LDS anyway) -- else on
    // wavefront 0
    // the team form exists for the 128-VGPR builds of the two symmetric stores with 32-bit counters, n <= 255; it caches the
    // utilities of the tour edges by position on wavefronts 0 .. ceil(n / 64) - 1, so the workgroup needs that many
    const bool team_exists = p.store != GLS_STORE_GLOBAL && p.penalty_bits == 32 && p.wps == 4 && n >= 4 && n <= 255 &&
                             p.threads / kWave >= (n + kWave - 1) / kWave;
    if (r.team_mode != 0 && team_exists) {
        const size_t lds = gls_lds_bytes(n, p.store, p.penalty_bits, true);
        // ... and only for the 16-wave workgroups that own a CU by their LDS footprint (distance triangle > 80 KB: n >= 144,
        // TSP200).  Measured (outer iterations in 2 s, team vs serial): TSP200 x 256 13.0k vs 10.9k (weight guide), 10.5k vs
        // 10.3k (regret_pred of the synthetic model), 6.7k vs 6.8k (noise); but TSP100 x 256 on 8-wave workgroups 20.3k vs
        // 24.2k (model guide) and TSP50 x 128 (one pass per scan) 18.3k vs 21.2k: a round's barriers, slot exchange and
        // the re-evaluation after a move cost more than the few passes they save (profiles/r03_experiments/README.md)
        // Round 5: the edge form of the serial phase (best improvement; gls_kernels.hip) beats the team form there too -- TSP200 x 256,
        // outer iterations in 2 s, serial edge form vs team: 18.4k vs 15.1k (model guide), 18.8k vs 17.2k (weight) -- so the
        // policy keeps the team form for first-improvement runs only (which have no edge form): profiles/r05_experiments/
        const bool pays = r.first_improvement && r.B > 0 && r.B <= r.num_cus && p.store == GLS_STORE_COMPACT && p.threads == 1024;
        if (lds <= kLdsPerCU && (r.team_mode == 1 || pays)) { p.team = true; p.lds = lds; }
    }
    const bool symmetric = p.store != GLS_STORE_GLOBAL;
    // + the pruned descent scans (nearest-neighbour lists: 2-opt scan from n = 80, relocate scan from n = 128; the position table
    // sits in the LDS slot the best tour used to have, so the footprint does not change); the lists must be full (n - 1 >= 32)
    p.prune = r.prune_mode != 0 && can_prune_of(r.first_improvement, symmetric, p.wps) && n >= kPruneMinNodes && n <= 255;
    p.gp = guide_passes(p, n);
    p.edge_form = edge_form_of(symmetric, p.penalty_bits / 8, r.first_improvement, p.team, p.wps);
    // counting instantiations (executed evaluations of the pruned scans): compact store, best improvement, 128-VGPR build,
    // no per-move trace.  A run that prunes AND asks for the executed-evaluation count must land on one: the others would
    // report executed == reference evaluations, a silently wrong ratio -- so elsewhere such a run cannot report it
    const bool can_count = p.store == GLS_STORE_COMPACT && p.wps == 4 && !r.first_improvement && !r.want_trace;
    p.count = r.want_count && p.prune && can_count;
    p.count_unknown = r.want_count && p.prune && !can_count;
    return p;
}

}  // namespace gnngls
