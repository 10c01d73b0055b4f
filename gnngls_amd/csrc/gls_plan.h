// gls_plan.h -- the launch plan of the persistent search kernel: which gls_kernel instantiation a run uses and how it is launched,
// as one value made by one pure function.  capi.hip makes the request, gls_kernels.hip turns the plan into a kernel (gls_kernel_fn).
#pragma once
#include <stddef.h>

#include "gls_policy.h"

namespace gnngls {

struct GlsRequest {
    int n, B;                  // nodes per instance; instances (0: no batch size known -- the capacity query)
    int penalty_bits;          // as given to gnngls_gls_run: 0 (auto), 16, 32, -1 (global-memory store), -2 (compact store)
    bool first_improvement, want_trace, want_count;    // want_count: the caller asks for the executed-evaluation count
    int num_cus;
    // experiment overrides (gnngls_debug_set_gls_team / _prune / _threads)
    int team_mode = -1;        // -1 = policy, 0 = never, 1 = wherever the team form exists
    int prune_mode = -1;       // -1 / 1 = pruned descent scans where they exist, 0 = full scans
    int threads_override = 0;  // 0 = policy
};

struct GlsPlan {
    int store, penalty_bits;   // GLS_STORE_*; counter width of the store (32 unless the uint16 LDS store)
    int threads; size_t lds;   // workgroup size, dynamic LDS bytes
    int per_cu;                // resident workgroups per CU
    int wps;                   // resident wavefronts per SIMD the instantiation is compiled for (512 / wps VGPRs)
    bool team;                 // perturbation phase on all wavefronts of the workgroup
    bool prune;                // the run builds neighbour lists and the descent scans prune with them
    bool first_improvement;
    int gp;                    // guide passes: register slots per lane for the tour edges (1, 2 or 4)
    bool trace;                // per-move trace
    bool count;                // counting instantiation (executed evaluations of the pruned scans)
    bool edge_form;            // serial perturbation phase in its edge form
    bool count_unknown;        // the run prunes on a build without the counting code: the caller reports -1
};

GlsPlan gls_plan(const GlsRequest &r);
size_t gls_lds_bytes(int n, int store, int penalty_bits, bool team = false);
// workgroup size by instance size and store (forced > 0: the experiment override); also sizes the unit kernels' workgroups
int gls_block_threads(int n, int store, int penalty_bits = 32, bool half_scans = true, int forced = 0);

}  // namespace gnngls
