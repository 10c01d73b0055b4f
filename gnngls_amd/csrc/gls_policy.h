// gls_policy.h -- what the search kernels (gls_kernels.hip) and the launch plan (gls_plan.cpp: plain host C++) both need: the
// build switches and thresholds the launch policy reads, and the two compile-time rules of the kernel the plan must agree with.
#pragma once
#include <stddef.h>

#ifndef GLS_WPS2
#define GLS_WPS2 1                   // 256-VGPR build of the one-slot kernel for batches of <= 2 single-wavefront workgroups per SIMD (TSP20 x 1000:
                                     // groups of 4 steps in the half-wave scans without scratch, +3 %; profiles/r04_experiments)
#endif
#ifndef GLS_PRUNE_MAX_WPS
#define GLS_PRUNE_MAX_WPS 6          // register budgets (waves per SIMD) whose instantiations carry the pruned descent scans: not the
                                     // 64-VGPR builds (batches of small instances: scratch 148 -> 100 B, +0.8 %; profiles/r04_experiments)
#endif
#ifndef GLS_HALF_SCANS
#define GLS_HALF_SCANS 1
#endif
#ifndef GLS_EDGE_PERTURB
#define GLS_EDGE_PERTURB 1           // 0: the scan-by-scan serial form everywhere (A/B builds)
#endif

namespace gnngls {

enum { GLS_STORE_GLOBAL = 0, GLS_STORE_TRI = 1, GLS_STORE_COMPACT = 2 };

constexpr size_t kLdsPerCU = 160 * 1024;   // LDS of a CU (MI355X)
constexpr int kWave = 64;
constexpr int kGuidePassesMax = 4;   // register-cached guide values cover n <= 256
constexpr int kHalfScanMinNodes = 8, kHalfScanMaxNodes = 33;
constexpr int kPruneMinNodes = 80;       // 2-opt scan pruned from here up (same-box A/B at n = 66 .. 127), relocate from n = 128
constexpr int kTriWavesPerSimd = 6, kCompactWavesPerSimd = 4, kGlobalWavesPerSimd = 4;     // the stores' default register budgets
// sizeof(Ctl), sizeof(TeamCtl): the LDS control blocks at the head of a workgroup's carve (asserted in gls_kernels.hip)
constexpr size_t kCtlBytes = 208, kTeamCtlBytes = 464;

// the edge form of the serial perturbation phase: best improvement, 32-bit counters, the 128-VGPR (and wider) builds
constexpr bool edge_form_of(bool symmetric, int pen_bytes, bool first_improvement, bool team, int wps) {
    return GLS_EDGE_PERTURB && symmetric && !first_improvement && !team && pen_bytes == 4 && wps <= 4;
}
// instantiations that carry the pruned descent scans (which then run where the launch hands them neighbour lists)
constexpr bool can_prune_of(bool first_improvement, bool symmetric, int wps) {
    return !first_improvement && symmetric && wps <= GLS_PRUNE_MAX_WPS;
}

}  // namespace gnngls
