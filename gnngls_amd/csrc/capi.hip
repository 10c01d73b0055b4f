// capi.hip -- extern "C" entry points of libgnngls_hip.so (declared in include/gnngls_hip.h).
// Argument checking, error strings and launch glue only; kernels live in gls_kernels.hip and
// model_kernels.hip.  No CPU fallback: every entry point either enqueues HIP work or fails.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <functional>
#include <mutex>
#include <vector>

#include "../../include/gnngls_hip.h"
#include "aco_kernels.h"
#include "alpha_kernels.h"
#include "beam_kernels.h"
#include "bounds_kernels.h"
#include "constructors_kernels.h"
#include "gls_kernels.h"
#include "greedy_edge_kernels.h"
#include "heads_kernels.h"
#include "labels_kernels.h"
#include "model_kernels.h"
#include "model_plan.h"
#include "oropt_kernels.h"
#include "sampling_kernels.h"
#include "threeopt_kernels.h"
#include "train_kernels.h"

namespace {
thread_local char g_err[512] = "";

int fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

int hip_fail(hipError_t e, const char *what) {
    return fail(GNNGLS_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
}

// ---- optional per-kernel-class timing with HIP events on the caller's stream -------------------
// (measurement hook for bench.py: process-global; the span log is guarded by a mutex so that concurrent callers on
// different host threads / streams may log safely; off unless gnngls_profile_enable(1) was called)
struct ProfSpan { int kind; hipEvent_t a, b; };
std::atomic<bool> g_prof_on{false};
std::mutex g_prof_mutex;
std::vector<ProfSpan> g_spans;

struct ProfScope {
    int kind; hipStream_t st; hipEvent_t a = nullptr;
    ProfScope(int k, hipStream_t s) : kind(k), st(s) {
        if (g_prof_on && hipEventCreate(&a) == hipSuccess) (void)hipEventRecord(a, st); else a = nullptr;
    }
    ~ProfScope() {
        if (!a) return;
        hipEvent_t b;
        if (hipEventCreate(&b) == hipSuccess) {
            (void)hipEventRecord(b, st);
            std::lock_guard<std::mutex> lock(g_prof_mutex);
            g_spans.push_back({kind, a, b});
        }
        else (void)hipEventDestroy(a);
    }
};

int g_pen16_limit = 65535;
// experiment overrides of the launch plan: they live here only and reach gls_plan() as plain fields of its request (plan_for)
std::atomic<int> g_prune_mode{-1};     // -1 / 1 = pruned descent scans where they exist, 0 = full scans (experiments / tests)
std::atomic<int> g_team_mode{-1};      // -1 = policy (gls_plan), 0 = never, 1 = wherever the team form exists (experiments / tests)
std::atomic<int> g_threads_override{0};      // experiments only (gnngls_debug_set_gls_threads)
long long *g_stamp_buffer = nullptr;
std::atomic<long long *> g_exec_evals{nullptr};   // measurement hook (gnngls_profile_set_executed_evals)

using gnngls::kLdsPerCU;

int num_cus() {
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0)
        return prop.multiProcessorCount;
    (void)hipGetLastError();
    return 256;   // MI355X
}

bool valid_penalty_bits(int bits) { return bits == 0 || bits == 16 || bits == 32 || bits == -1 || bits == -2; }

// the plan of a search of B instances of n nodes on the current device, under the overrides as they are now
gnngls::GlsPlan plan_for(int n, int B, int penalty_bits, bool first_improvement, bool want_trace = false, bool want_count = false) {
    return gnngls::gls_plan({n, B, penalty_bits, first_improvement, want_trace, want_count, num_cus(), g_team_mode.load(std::memory_order_relaxed),
                             g_prune_mode.load(std::memory_order_relaxed), g_threads_override.load(std::memory_order_relaxed)});
}

// gnngls_gls_describe_run, and with fewer outputs gnngls_gls_describe_config
int describe_plan(const char *what, int n, int B, int penalty_bits, bool first_improvement, int *store, int *threads, int *lds_bytes,
                  int *per_cu, int *waves_per_simd = nullptr, int *team = nullptr, int *edge_form = nullptr) {
    if (n < 3 || B < 0 || !valid_penalty_bits(penalty_bits)) return fail(GNNGLS_ERR_ARG, "%s: bad argument", what);
    const gnngls::GlsPlan c = plan_for(n, B, penalty_bits, first_improvement);      // exactly what gnngls_gls_run launches
    if (c.lds > kLdsPerCU)
        return fail(GNNGLS_ERR_UNSUPPORTED, "%s: n=%d needs %zu B of LDS for tours and edge lengths (> 160 KiB)", what, n, c.lds);
    if (store) *store = c.store * 100 + (c.store == gnngls::GLS_STORE_TRI ? c.penalty_bits : 0);
    if (threads) *threads = c.threads;
    if (lds_bytes) *lds_bytes = (int)c.lds;
    if (per_cu) *per_cu = c.store == gnngls::GLS_STORE_GLOBAL ? 0 : c.per_cu;
    if (waves_per_simd) *waves_per_simd = c.wps;
    if (team) *team = c.team ? 1 : 0;
    if (edge_form) *edge_form = c.edge_form ? 1 : 0;
    return GNNGLS_OK;
}

// stream-ordered scratch: freed on the stream it was allocated on when the scope ends, behind what the scope enqueued
struct StreamScratch {
    void *p = nullptr; hipStream_t st;
    explicit StreamScratch(hipStream_t s) : st(s) {}
    StreamScratch(const StreamScratch &) = delete;
    ~StreamScratch() { if (p) (void)hipFreeAsync(p, st); }
    hipError_t alloc(size_t bytes) {
        const hipError_t e = hipMallocAsync(&p, bytes, st);
        if (e != hipSuccess) p = nullptr;
        return e;
    }
};
}  // namespace

extern "C" {

int gnngls_abi_version(void) { return 4; }
const char *gnngls_last_error(void) { return g_err; }

int gnngls_gls_resident_capacity(int n) {
    if (n < 3) return 0;
    const gnngls::GlsPlan c = plan_for(n, 0, 0, false);
    if (c.store == gnngls::GLS_STORE_GLOBAL) return 0;
    return c.per_cu * num_cus();
}

int gnngls_gls_describe_config(int n, int B, int penalty_bits, int *store, int *threads, int *lds_bytes, int *per_cu) {
    return describe_plan("gls_describe_config", n, B, penalty_bits, false, store, threads, lds_bytes, per_cu);     // as a best-improvement run would be launched
}

int gnngls_gls_describe_run(int n, int B, int penalty_bits, int first_improvement, int *store, int *threads, int *lds_bytes,
                            int *per_cu, int *waves_per_simd, int *team, int *edge_form) {
    return describe_plan("gls_describe_run", n, B, penalty_bits, first_improvement != 0, store, threads, lds_bytes, per_cu, waves_per_simd,
                         team, edge_form);
}

int gnngls_gls_kernel_resources(int n, int B, int penalty_bits, int first_improvement, int trace, int *vgprs, int *scratch_bytes) {
    if (n < 3 || B < 0 || !valid_penalty_bits(penalty_bits)) return fail(GNNGLS_ERR_ARG, "gls_kernel_resources: bad argument");
    const hipError_t e = gnngls::gls_kernel_resources(plan_for(n, B, penalty_bits, first_improvement != 0, trace != 0), vgprs, scratch_bytes);
    return e == hipSuccess ? GNNGLS_OK : hip_fail(e, "gls_kernel_resources");
}

int gnngls_gls_waves_per_simd(int n, int B, int penalty_bits) {
    if (n < 3 || B < 0 || !valid_penalty_bits(penalty_bits)) return 0;
    return plan_for(n, B, penalty_bits, false).wps;
}

int gnngls_gls_uses_team(int n, int B, int penalty_bits) {
    if (n < 3 || B < 0 || !valid_penalty_bits(penalty_bits)) return 0;
    return plan_for(n, B, penalty_bits, false).team ? 1 : 0;
}

int gnngls_two_opt_delta_all(const int32_t *tour, const double *D, int B, int n, double *out, void *stream) {
    if (B == 0) return GNNGLS_OK;   // empty batch: nothing to enqueue (data pointers may be NULL)
    if (!tour || !D || !out || B < 0 || n < 3) return fail(GNNGLS_ERR_ARG, "two_opt_delta_all: bad argument");
    hipError_t e = gnngls::launch_delta_all(tour, D, B, n, 0, out, (hipStream_t)stream);
    return e == hipSuccess ? GNNGLS_OK : hip_fail(e, "two_opt_delta_all");
}

int gnngls_relocate_delta_all(const int32_t *tour, const double *D, int B, int n, double *out, void *stream) {
    if (B == 0) return GNNGLS_OK;   // empty batch: nothing to enqueue (data pointers may be NULL)
    if (!tour || !D || !out || B < 0 || n < 3) return fail(GNNGLS_ERR_ARG, "relocate_delta_all: bad argument");
    hipError_t e = gnngls::launch_delta_all(tour, D, B, n, 1, out, (hipStream_t)stream);
    return e == hipSuccess ? GNNGLS_OK : hip_fail(e, "relocate_delta_all");
}

int gnngls_best_move(const int32_t *tour, const double *D, int B, int n, int op, const int32_t *pos_i,
                     int first_improvement, double *delta_out, int32_t *move_out, int32_t *new_tour, void *stream) {
    if (B == 0) return GNNGLS_OK;   // empty batch: nothing to enqueue (data pointers may be NULL)
    if (!tour || !D || !delta_out || !move_out || B < 0 || n < 3 || (op != 0 && op != 1) || n > 65535)
        return fail(GNNGLS_ERR_ARG, "best_move: bad argument");
    const int threads = gnngls::gls_block_threads(n, gnngls::GLS_STORE_GLOBAL, 32, true, g_threads_override.load(std::memory_order_relaxed));
    hipError_t e = gnngls::launch_best_move(tour, D, B, n, op, pos_i, first_improvement != 0, threads, delta_out, move_out,
                                            new_tour, (hipStream_t)stream);
    return e == hipSuccess ? GNNGLS_OK : hip_fail(e, "best_move");
}

int gnngls_tour_cost(const int32_t *tour, const double *D, int B, int n, double *cost_out, void *stream) {
    if (B == 0) return GNNGLS_OK;   // empty batch: nothing to enqueue (data pointers may be NULL)
    if (!tour || !D || !cost_out || B < 0 || n < 1) return fail(GNNGLS_ERR_ARG, "tour_cost: bad argument");
    ProfScope ps(GNNGLS_PROF_TOUR_COST, (hipStream_t)stream);
    hipError_t e = gnngls::launch_tour_cost(tour, D, B, n, cost_out, (hipStream_t)stream);
    return e == hipSuccess ? GNNGLS_OK : hip_fail(e, "tour_cost");
}

int gnngls_nearest_neighbor(const double *W, int B, int n, int depot, int32_t *tour_out, void *stream) {
    if (B == 0) return GNNGLS_OK;   // empty batch: nothing to enqueue (data pointers may be NULL)
    if (!W || !tour_out || B < 0 || n < 1 || depot < 0 || depot >= n)
        return fail(GNNGLS_ERR_ARG, "nearest_neighbor: bad argument");
    ProfScope ps(GNNGLS_PROF_NEAREST_NEIGHBOR, (hipStream_t)stream);
    hipError_t e = gnngls::launch_nearest_neighbor(W, B, n, depot, tour_out, (hipStream_t)stream);
    return e == hipSuccess ? GNNGLS_OK : hip_fail(e, "nearest_neighbor");
}

static_assert(GNNGLS_INSERTION_MAX_N == gnngls::kInsertionMaxN, "include/gnngls_hip.h and constructors_kernels.h disagree");

int gnngls_insertion(const double *W, int B, int n, int depot, int mode, const int32_t *order, int32_t *tour_out,
                     int32_t *status, void *stream) {
    if (B == 0) return GNNGLS_OK;
    if (!W || !tour_out) return fail(GNNGLS_ERR_ARG, "insertion: NULL pointer (W, tour_out)");
    if (B < 0) return fail(GNNGLS_ERR_ARG, "insertion: B=%d must be >= 0", B);
    if (n < 1) return fail(GNNGLS_ERR_ARG, "insertion: n=%d must be >= 1", n);
    if (depot < 0 || depot >= n) return fail(GNNGLS_ERR_ARG, "insertion: depot=%d out of range (0..%d)", depot, n - 1);
    if (mode != GNNGLS_INSERT_NEAREST && mode != GNNGLS_INSERT_FARTHEST && mode != GNNGLS_INSERT_GIVEN_ORDER)
        return fail(GNNGLS_ERR_ARG, "insertion: unknown mode %d", mode);
    if (mode == GNNGLS_INSERT_GIVEN_ORDER && (!status || (!order && n > 1)))
        return fail(GNNGLS_ERR_ARG, "insertion: mode GNNGLS_INSERT_GIVEN_ORDER needs order and status");
    if (n > GNNGLS_INSERTION_MAX_N)
        return fail(GNNGLS_ERR_UNSUPPORTED, "insertion: n=%d exceeds the largest supported instance (n <= %d: the tour state of an instance lives in LDS)",
                    n, GNNGLS_INSERTION_MAX_N);
    ProfScope ps(GNNGLS_PROF_INSERTION, (hipStream_t)stream);
    hipError_t e = gnngls::launch_insertion(W, B, n, depot, mode, order, tour_out, status, (hipStream_t)stream);
    return e == hipSuccess ? GNNGLS_OK : hip_fail(e, "insertion");
}

int gnngls_cheapest_insertion(const int32_t *sub_tour, int len, const int32_t *node, const double *W, int B, int n,
                              int32_t *tour_out, double *cost_out, void *stream) {
    if (B == 0) return GNNGLS_OK;
    if (!sub_tour || !node || !W || !tour_out || !cost_out) return fail(GNNGLS_ERR_ARG, "cheapest_insertion: NULL pointer");
    if (B < 0) return fail(GNNGLS_ERR_ARG, "cheapest_insertion: B=%d must be >= 0", B);
    if (n < 1) return fail(GNNGLS_ERR_ARG, "cheapest_insertion: n=%d must be >= 1", n);
    if (len < 2 || len > n) return fail(GNNGLS_ERR_ARG, "cheapest_insertion: len=%d out of range (2..n=%d)", len, n);
    if (n > GNNGLS_INSERTION_MAX_N)
        return fail(GNNGLS_ERR_UNSUPPORTED, "cheapest_insertion: n=%d exceeds the largest supported instance (n <= %d)", n,
                    GNNGLS_INSERTION_MAX_N);
    ProfScope ps(GNNGLS_PROF_INSERTION, (hipStream_t)stream);
    hipError_t e = gnngls::launch_cheapest_insertion(sub_tour, len, node, W, B, n, tour_out, cost_out, (hipStream_t)stream);
    return e == hipSuccess ? GNNGLS_OK : hip_fail(e, "cheapest_insertion");
}

static_assert(GNNGLS_ONE_TREE_MAX_N == gnngls::kOneTreeMaxN, "include/gnngls_hip.h and bounds_kernels.h disagree");
static_assert(GNNGLS_BOUND_EXIT_ITERS == gnngls::BOUND_EXIT_ITERS && GNNGLS_BOUND_EXIT_STEP == gnngls::BOUND_EXIT_STEP &&
              GNNGLS_BOUND_EXIT_TOUR == gnngls::BOUND_EXIT_TOUR && GNNGLS_STATUS_ASYMMETRIC == GNNGLS_STATUS_ASYMMETRIC_DEV,
              "include/gnngls_hip.h and bounds_kernels.h disagree");

int gnngls_one_tree_bound(const double *D, const double *ub, int B, int n, int max_iters, double *bound, double *pi, int32_t *iters,
                          int32_t *exit_kind, int32_t *status, void *stream) {
    if (B < 0) return fail(GNNGLS_ERR_ARG, "one_tree_bound: B=%d must be >= 0", B);
    if (n < 3) return fail(GNNGLS_ERR_ARG, "one_tree_bound: n=%d must be >= 3", n);
    if (n > GNNGLS_ONE_TREE_MAX_N)
        return fail(GNNGLS_ERR_UNSUPPORTED, "one_tree_bound: n=%d exceeds the largest supported instance (n <= %d: the ascent state of an "
                    "instance lives in the registers of one workgroup)", n, GNNGLS_ONE_TREE_MAX_N);
    if (max_iters < 0) return fail(GNNGLS_ERR_ARG, "one_tree_bound: max_iters=%d must be >= 0", max_iters);
    if (B == 0) return GNNGLS_OK;
    if (!D || !ub || !bound || !iters || !exit_kind || !status)
        return fail(GNNGLS_ERR_ARG, "one_tree_bound: NULL pointer (D, ub, bound, iters, exit_kind, status)");
    ProfScope ps(GNNGLS_PROF_ONE_TREE_BOUND, (hipStream_t)stream);
    hipError_t e = gnngls::launch_one_tree_bound(D, ub, B, n, max_iters, bound, pi, iters, exit_kind, status, (hipStream_t)stream);
    return e == hipSuccess ? GNNGLS_OK : hip_fail(e, "one_tree_bound");
}

int gnngls_one_tree_bound_describe(int n, int *threads, int *lds_bytes, int *nodes_per_lane) {
    if (n < 3 || n > GNNGLS_ONE_TREE_MAX_N) return fail(GNNGLS_ERR_ARG, "one_tree_bound_describe: n=%d out of range (3..%d)", n, GNNGLS_ONE_TREE_MAX_N);
    const int t = gnngls::one_tree_threads(n);
    if (threads) *threads = t;
    if (lds_bytes) *lds_bytes = gnngls::one_tree_lds_bytes(n);
    if (nodes_per_lane) *nodes_per_lane = t > 64 ? 4 : (n + 63) / 64;
    return GNNGLS_OK;
}

static_assert(GNNGLS_ALPHA_MAX_N == gnngls::kAlphaMaxN && GNNGLS_STATUS_ASYMMETRIC == gnngls::kAlphaStatusAsymmetric,
              "include/gnngls_hip.h and alpha_kernels.h disagree");

int gnngls_alpha_nearness(const double *D, const double *pi, int B, int n, double *alpha, int32_t *status, void *stream) {
    if (B < 1) return fail(GNNGLS_ERR_ARG, "alpha_nearness: B=%d must be >= 1", B);
    if (n < 3) return fail(GNNGLS_ERR_ARG, "alpha_nearness: n=%d must be >= 3", n);
    if (n > GNNGLS_ALPHA_MAX_N)
        return fail(GNNGLS_ERR_UNSUPPORTED, "alpha_nearness: n=%d exceeds the largest supported instance (n <= %d: the Prim state of an "
                    "instance lives in the registers of one workgroup)", n, GNNGLS_ALPHA_MAX_N);
    if (!D || !alpha || !status) return fail(GNNGLS_ERR_ARG, "alpha_nearness: NULL pointer (D, alpha, status)");
    hipError_t e = gnngls::launch_alpha_nearness(D, pi, B, n, alpha, status, (hipStream_t)stream);
    return e == hipSuccess ? GNNGLS_OK : hip_fail(e, "alpha_nearness");
}

static_assert(GNNGLS_OR_OPT_MAX_N == gnngls::kOrOptMaxN && GNNGLS_OR_OPT_MAX_SEG == gnngls::kOrOptMaxSeg &&
              GNNGLS_STATUS_ASYMMETRIC == gnngls::kOrOptStatusAsymmetric && GNNGLS_STATUS_MOVE_CAP == gnngls::kOrOptStatusMoveCap,
              "include/gnngls_hip.h and oropt_kernels.h disagree");

// the checks both Or-opt entries share; 0 = the arguments are fine
static int or_opt_args(const char *what, int B, int n, int max_seg) {
    if (B < 1) return fail(GNNGLS_ERR_ARG, "%s: B=%d must be >= 1", what, B);
    if (n < 3) return fail(GNNGLS_ERR_ARG, "%s: n=%d must be >= 3", what, n);
    if (n > GNNGLS_OR_OPT_MAX_N)
        return fail(GNNGLS_ERR_UNSUPPORTED, "%s: n=%d exceeds the largest supported instance (n <= %d: a move's selection key holds "
                    "its positions in ten bits each)", what, n, GNNGLS_OR_OPT_MAX_N);
    if (max_seg < 1 || max_seg > GNNGLS_OR_OPT_MAX_SEG)
        return fail(GNNGLS_ERR_ARG, "%s: max_seg=%d must be in 1..%d", what, max_seg, GNNGLS_OR_OPT_MAX_SEG);
    return GNNGLS_OK;
}

int gnngls_or_opt_best_move(const int32_t *tour, const double *D, int B, int n, int max_seg, int reverse, double *delta,
                            int32_t *move, int32_t *new_tour, void *stream) {
    if (int rc = or_opt_args("or_opt_best_move", B, n, max_seg)) return rc;
    if (!tour || !D || !delta || !move || !new_tour)
        return fail(GNNGLS_ERR_ARG, "or_opt_best_move: NULL pointer (tour, D, delta, move, new_tour)");
    hipError_t e = gnngls::launch_or_opt_best_move(tour, D, B, n, max_seg, reverse, delta, move, new_tour, (hipStream_t)stream);
    return e == hipSuccess ? GNNGLS_OK : hip_fail(e, "or_opt_best_move");
}

int gnngls_or_opt_descent(const int32_t *tour, const double *cost, const double *D, int B, int n, int max_seg, int reverse,
                          int max_moves, int32_t *tour_out, double *cost_out, int32_t *moves, int32_t *status, double *trace_cost,
                          int trace_cap, void *stream) {
    if (int rc = or_opt_args("or_opt_descent", B, n, max_seg)) return rc;
    if (max_moves < 1) return fail(GNNGLS_ERR_ARG, "or_opt_descent: max_moves=%d must be >= 1 (it bounds the loop)", max_moves);
    if (trace_cap < 0) return fail(GNNGLS_ERR_ARG, "or_opt_descent: trace_cap=%d must be >= 0", trace_cap);
    if (!tour || !cost || !D || !tour_out || !cost_out || !moves || !status)
        return fail(GNNGLS_ERR_ARG, "or_opt_descent: NULL pointer (tour, cost, D, tour_out, cost_out, moves, status)");
    hipError_t e = gnngls::launch_or_opt_descent(tour, cost, D, B, n, max_seg, reverse, max_moves, tour_out, cost_out, moves, status,
                                                 trace_cost, trace_cost ? trace_cap : 0, (hipStream_t)stream);
    return e == hipSuccess ? GNNGLS_OK : hip_fail(e, "or_opt_descent");
}

int gnngls_ils_run(const int32_t *tour, const double *cost, const double *D, int B, int n, int kicks, int kick0, int max_seg, int reverse,
                   int max_moves, uint64_t seed, const double *u, int32_t *tour_out, double *cost_out, int32_t *moves, int32_t *accepted,
                   int32_t *status, double *trace_cost, void *stream) {
    if (n < 4) return fail(GNNGLS_ERR_ARG, "ils_run: n=%d must be >= 4 (a double bridge cuts the tour into four pieces)", n);
    if (int rc = or_opt_args("ils_run", B, n, max_seg)) return rc;
    if (kicks < 0) return fail(GNNGLS_ERR_ARG, "ils_run: kicks=%d must be >= 0", kicks);
    if (kick0 < 0) return fail(GNNGLS_ERR_ARG, "ils_run: kick0=%d must be >= 0", kick0);
    if ((long long)kick0 + kicks > 0x7fffffffLL)
        return fail(GNNGLS_ERR_ARG, "ils_run: kick0 + kicks = %lld exceeds 2^31 - 1 (the kick counter)", (long long)kick0 + kicks);
    if (max_moves < 1) return fail(GNNGLS_ERR_ARG, "ils_run: max_moves=%d must be >= 1 (with kicks it bounds the loop)", max_moves);
    if (!tour || !cost || !D || !tour_out || !cost_out || !moves || !accepted || !status)
        return fail(GNNGLS_ERR_ARG, "ils_run: NULL pointer (tour, cost, D, tour_out, cost_out, moves, accepted, status)");
    hipError_t e = gnngls::launch_ils(tour, cost, D, B, n, kicks, kick0, max_seg, reverse, max_moves, seed, u, tour_out, cost_out, moves,
                                      accepted, status, trace_cost, (hipStream_t)stream);
    return e == hipSuccess ? GNNGLS_OK : hip_fail(e, "ils_run");
}

static_assert(GNNGLS_STATUS_STEP_CAP == gnngls::kGuidedStatusStepCap, "include/gnngls_hip.h and oropt_kernels.h disagree");

int gnngls_or_opt_o2a(const int32_t *tour, const double *D, const int32_t *pos, int B, int n, int max_seg, int reverse, double *delta,
                      int32_t *move, int32_t *new_tour, void *stream) {
    if (int rc = or_opt_args("or_opt_o2a", B, n, max_seg)) return rc;
    if (!tour || !D || !pos || !delta || !move || !new_tour)
        return fail(GNNGLS_ERR_ARG, "or_opt_o2a: NULL pointer (tour, D, pos, delta, move, new_tour)");
    hipError_t e = gnngls::launch_or_opt_o2a(tour, D, pos, B, n, max_seg, reverse, delta, move, new_tour, (hipStream_t)stream);
    return e == hipSuccess ? GNNGLS_OK : hip_fail(e, "or_opt_o2a");
}

int gnngls_guided_or_opt_run(const int32_t *tour, const double *cost, const double *D, const double *guides, int G, const double *k,
                             int32_t *penalty, int B, int n, int outer_iters, int iter0, int perturbation_moves, int max_seg,
                             int reverse, int max_moves, int max_steps, int32_t *tour_out, double *cost_out, int32_t *best_tour,
                             double *best_cost, int32_t *moves, int32_t *steps, int32_t *status, double *trace_cost, int trace_cap,
                             int32_t *trace_len, void *stream) {
    if (n < 4) return fail(GNNGLS_ERR_ARG, "guided_or_opt_run: n=%d must be >= 4", n);
    if (int rc = or_opt_args("guided_or_opt_run", B, n, max_seg)) return rc;
    if (outer_iters < 0) return fail(GNNGLS_ERR_ARG, "guided_or_opt_run: outer_iters=%d must be >= 0", outer_iters);
    if (iter0 < 0) return fail(GNNGLS_ERR_ARG, "guided_or_opt_run: iter0=%d must be >= 0", iter0);
    if ((long long)iter0 + outer_iters > 0x7fffffffLL)
        return fail(GNNGLS_ERR_ARG, "guided_or_opt_run: iter0 + outer_iters = %lld exceeds 2^31 - 1 (the guide index)",
                    (long long)iter0 + outer_iters);
    if (outer_iters > 0 && (G < 1 || !guides))
        return fail(GNNGLS_ERR_ARG, "guided_or_opt_run: outer_iters=%d needs guides (G=%d, guides %s)", outer_iters, G,
                    guides ? "given" : "NULL");
    if (perturbation_moves < 0)
        return fail(GNNGLS_ERR_ARG, "guided_or_opt_run: perturbation_moves=%d must be >= 0", perturbation_moves);
    if (max_moves < 1) return fail(GNNGLS_ERR_ARG, "guided_or_opt_run: max_moves=%d must be >= 1 (it bounds the run)", max_moves);
    if (max_steps < 1) return fail(GNNGLS_ERR_ARG, "guided_or_opt_run: max_steps=%d must be >= 1 (it bounds the run)", max_steps);
    if (trace_cap < 0) return fail(GNNGLS_ERR_ARG, "guided_or_opt_run: trace_cap=%d must be >= 0", trace_cap);
    if (!tour || !cost || !D || !k || !penalty || !tour_out || !cost_out || !best_tour || !best_cost || !moves || !steps || !status)
        return fail(GNNGLS_ERR_ARG, "guided_or_opt_run: NULL pointer (tour, cost, D, k, penalty, tour_out, cost_out, best_tour, "
                    "best_cost, moves, steps, status)");
    hipError_t e = gnngls::launch_guided_or_opt(tour, cost, D, guides, G > 0 ? G : 1, k, penalty, B, n, outer_iters, iter0,
                                                perturbation_moves, max_seg, reverse, max_moves, max_steps, tour_out, cost_out,
                                                best_tour, best_cost, moves, steps, status, trace_cost, trace_cost ? trace_cap : 0,
                                                trace_len, (hipStream_t)stream);
    return e == hipSuccess ? GNNGLS_OK : hip_fail(e, "guided_or_opt_run");
}

static_assert(GNNGLS_THREE_OPT_MAX_N == gnngls::kThreeOptMaxN && GNNGLS_STATUS_ASYMMETRIC == gnngls::kThreeOptStatusAsymmetric &&
              GNNGLS_STATUS_MOVE_CAP == gnngls::kThreeOptStatusMoveCap, "include/gnngls_hip.h and threeopt_kernels.h disagree");

// the checks both 3-opt entries share; 0 = the arguments are fine
static int three_opt_args(const char *what, int B, int n) {
    if (B < 1) return fail(GNNGLS_ERR_ARG, "%s: B=%d must be >= 1", what, B);
    if (n < 3) return fail(GNNGLS_ERR_ARG, "%s: n=%d must be >= 3", what, n);
    if (n > GNNGLS_THREE_OPT_MAX_N)
        return fail(GNNGLS_ERR_UNSUPPORTED, "%s: n=%d exceeds the largest supported instance (n <= %d: a move's selection key holds "
                    "its positions in eight bits each)", what, n, GNNGLS_THREE_OPT_MAX_N);
    return GNNGLS_OK;
}

int gnngls_three_opt_best_move(const int32_t *tour, const double *D, int B, int n, double *delta, int32_t *move, int32_t *new_tour,
                               void *stream) {
    if (int rc = three_opt_args("three_opt_best_move", B, n)) return rc;
    if (!tour || !D || !delta || !move || !new_tour)
        return fail(GNNGLS_ERR_ARG, "three_opt_best_move: NULL pointer (tour, D, delta, move, new_tour)");
    hipError_t e = gnngls::launch_three_opt_best_move(tour, D, B, n, delta, move, new_tour, (hipStream_t)stream);
    return e == hipSuccess ? GNNGLS_OK : hip_fail(e, "three_opt_best_move");
}

int gnngls_three_opt_descent(const int32_t *tour, const double *cost, const double *D, int B, int n, int max_moves, int32_t *tour_out,
                             double *cost_out, int32_t *moves, int32_t *status, double *trace_cost, int trace_cap, void *stream) {
    if (int rc = three_opt_args("three_opt_descent", B, n)) return rc;
    if (max_moves < 1) return fail(GNNGLS_ERR_ARG, "three_opt_descent: max_moves=%d must be >= 1 (it bounds the loop)", max_moves);
    if (trace_cap < 0) return fail(GNNGLS_ERR_ARG, "three_opt_descent: trace_cap=%d must be >= 0", trace_cap);
    if (!tour || !cost || !D || !tour_out || !cost_out || !moves || !status)
        return fail(GNNGLS_ERR_ARG, "three_opt_descent: NULL pointer (tour, cost, D, tour_out, cost_out, moves, status)");
    if (!trace_cost && trace_cap > 0)
        return fail(GNNGLS_ERR_ARG, "three_opt_descent: NULL pointer (trace_cost) with trace_cap=%d (NULL only with trace_cap 0)", trace_cap);
    hipError_t e = gnngls::launch_three_opt_descent(tour, cost, D, B, n, max_moves, tour_out, cost_out, moves, status, trace_cost,
                                                    trace_cap, (hipStream_t)stream);
    return e == hipSuccess ? GNNGLS_OK : hip_fail(e, "three_opt_descent");
}

int gnngls_three_opt_lds_max_n(void) { return gnngls::three_opt_lds_max_n(); }

static_assert(GNNGLS_SAMPLE_MAX_N == gnngls::kSampleMaxN && GNNGLS_SAMPLE_BAD_WEIGHTS == GNNGLS_SAMPLE_BAD_WEIGHTS_DEV,
              "include/gnngls_hip.h and sampling_kernels.h disagree");

int gnngls_sample_nn_tours(const double *W, int B, int n, int R, int depot, int invert, uint64_t seed, const double *u,
                           int32_t *tours, int32_t *status, void *stream) {
    if (B < 0) return fail(GNNGLS_ERR_ARG, "sample_nn_tours: B=%d must be >= 0", B);
    if (n < 3) return fail(GNNGLS_ERR_ARG, "sample_nn_tours: n=%d must be >= 3", n);
    if (n > GNNGLS_SAMPLE_MAX_N)
        return fail(GNNGLS_ERR_UNSUPPORTED, "sample_nn_tours: n=%d exceeds the largest supported instance (n <= %d: the state of a walk "
                    "lives in the registers of one wavefront)", n, GNNGLS_SAMPLE_MAX_N);
    if (R < 1) return fail(GNNGLS_ERR_ARG, "sample_nn_tours: R=%d must be >= 1", R);
    if (depot < 0 || depot >= n) return fail(GNNGLS_ERR_ARG, "sample_nn_tours: depot=%d out of range (0..%d)", depot, n - 1);
    if ((long long)B * R > 0x7fffffffLL) return fail(GNNGLS_ERR_ARG, "sample_nn_tours: B * R = %lld walks exceed 2^31 - 1", (long long)B * R);
    if (B == 0) return GNNGLS_OK;
    if (!W || !tours || !status) return fail(GNNGLS_ERR_ARG, "sample_nn_tours: NULL pointer (W, tours, status)");
    hipError_t e = gnngls::launch_sample_nn_tours(W, B, n, R, depot, invert != 0, seed, u, tours, status, (hipStream_t)stream);
    return e == hipSuccess ? GNNGLS_OK : hip_fail(e, "sample_nn_tours");
}

static_assert(GNNGLS_ACO_MAX_N == gnngls::kAcoMaxN && GNNGLS_ACO_MAX_ANTS == gnngls::kAcoMaxAnts &&
              GNNGLS_SAMPLE_BAD_WEIGHTS == gnngls::kAcoStatusBadWeights, "include/gnngls_hip.h and aco_kernels.h disagree");

int gnngls_aco_run(const double *D, const double *H, double *tau, int32_t *best_tour, double *best_cost, int B, int n, int ants, int iters,
                   int64_t iter0, double rho, double min_ratio, int gb_every, int spread_starts, uint64_t seed, const double *u,
                   int32_t *iters_done, int32_t *status, double *trace_cost, int32_t *ant_tours, double *ant_cost, void *stream) {
    if (B < 1) return fail(GNNGLS_ERR_ARG, "aco_run: B=%d must be >= 1", B);
    if (n < 3) return fail(GNNGLS_ERR_ARG, "aco_run: n=%d must be >= 3", n);
    if (n > GNNGLS_ACO_MAX_N)
        return fail(GNNGLS_ERR_UNSUPPORTED, "aco_run: n=%d exceeds the largest supported instance (n <= %d: the state of a walk lives in "
                    "the registers of one wavefront)", n, GNNGLS_ACO_MAX_N);
    if (ants < 1) return fail(GNNGLS_ERR_ARG, "aco_run: ants=%d must be >= 1", ants);
    if (ants > GNNGLS_ACO_MAX_ANTS)
        return fail(GNNGLS_ERR_UNSUPPORTED, "aco_run: ants=%d exceeds the largest supported colony (ants <= %d)", ants, GNNGLS_ACO_MAX_ANTS);
    if (iters < 0) return fail(GNNGLS_ERR_ARG, "aco_run: iters=%d must be >= 0", iters);
    if (iter0 < 0) return fail(GNNGLS_ERR_ARG, "aco_run: iter0=%lld must be >= 0", (long long)iter0);
    if (iter0 > 0xffffffffLL || (iter0 + iters) * (long long)ants > 0xffffffffLL)
        return fail(GNNGLS_ERR_ARG, "aco_run: (iter0 + iters) * ants = (%lld + %d) * %d must stay below 2^32 (the walk counter of the "
                    "generator)", (long long)iter0, iters, ants);
    if (!(rho > 0.0 && rho < 1.0)) return fail(GNNGLS_ERR_ARG, "aco_run: rho=%g must be in (0, 1)", rho);
    if (!(min_ratio > 0.0 && min_ratio <= 1.0)) return fail(GNNGLS_ERR_ARG, "aco_run: min_ratio=%g must be in (0, 1]", min_ratio);
    if (gb_every < 0) return fail(GNNGLS_ERR_ARG, "aco_run: gb_every=%d must be >= 0", gb_every);
    if (!D || !H || !tau || !best_tour || !best_cost || !iters_done || !status)
        return fail(GNNGLS_ERR_ARG, "aco_run: NULL pointer (D, H, tau, best_tour, best_cost, iters_done, status)");
    if ((ant_tours == nullptr) != (ant_cost == nullptr))
        return fail(GNNGLS_ERR_ARG, "aco_run: NULL pointer (ant_tours and ant_cost are given together or not at all)");
    hipError_t e = gnngls::launch_aco(D, H, tau, best_tour, best_cost, B, n, ants, iters, (long long)iter0, rho, min_ratio, gb_every,
                                      spread_starts != 0, seed, u, iters_done, status, trace_cost, ant_tours, ant_cost,
                                      (hipStream_t)stream);
    return e == hipSuccess ? GNNGLS_OK : hip_fail(e, "aco_run");
}

static_assert(GNNGLS_BEAM_MAX_N == gnngls::kBeamMaxN && GNNGLS_BEAM_MAX_WIDTH == gnngls::kBeamMaxWidth &&
              GNNGLS_BEAM_BAD_SCORE == gnngls::kBeamStatusBadScore, "include/gnngls_hip.h and beam_kernels.h disagree");

int64_t gnngls_beam_search_workspace_bytes(int B, int n, int width) {
    if (B < 1 || n < 3 || n > GNNGLS_BEAM_MAX_N || width < 1 || width > GNNGLS_BEAM_MAX_WIDTH) return 0;
    return (int64_t)gnngls::beam_workspace_bytes(B, n, width);
}

int gnngls_beam_search(const double *S, const double *D, int B, int n, int width, int depot, int select, int32_t *best_tour,
                       double *best_score, double *best_cost, int32_t *n_beams, int32_t *status, int32_t *beam_tours,
                       double *beam_score, double *beam_cost, void *workspace, int64_t workspace_bytes, void *stream) {
    if (B < 1) return fail(GNNGLS_ERR_ARG, "beam_search: B=%d must be >= 1", B);
    if (n < 3) return fail(GNNGLS_ERR_ARG, "beam_search: n=%d must be >= 3", n);
    if (n > GNNGLS_BEAM_MAX_N)
        return fail(GNNGLS_ERR_UNSUPPORTED, "beam_search: n=%d exceeds the largest supported instance (n <= %d: a back-pointer packs the "
                    "node into 10 bits)", n, GNNGLS_BEAM_MAX_N);
    if (width < 1) return fail(GNNGLS_ERR_ARG, "beam_search: width=%d must be >= 1", width);
    if (width > GNNGLS_BEAM_MAX_WIDTH)
        return fail(GNNGLS_ERR_UNSUPPORTED, "beam_search: width=%d exceeds the widest supported beam (width <= %d)", width,
                    GNNGLS_BEAM_MAX_WIDTH);
    if (depot < 0 || depot >= n) return fail(GNNGLS_ERR_ARG, "beam_search: depot=%d must be in [0, %d)", depot, n);
    if (select != GNNGLS_BEAM_SELECT_SCORE && select != GNNGLS_BEAM_SELECT_COST)
        return fail(GNNGLS_ERR_ARG, "beam_search: select=%d must be %d (score) or %d (cost)", select, GNNGLS_BEAM_SELECT_SCORE,
                    GNNGLS_BEAM_SELECT_COST);
    if (select == GNNGLS_BEAM_SELECT_COST && !D) return fail(GNNGLS_ERR_ARG, "beam_search: select=cost needs the distances D");
    if (!S || !best_tour || !best_score || !best_cost || !n_beams || !status)
        return fail(GNNGLS_ERR_ARG, "beam_search: NULL pointer (S, best_tour, best_score, best_cost, n_beams, status)");
    if ((beam_tours == nullptr) != (beam_score == nullptr) || (beam_tours == nullptr) != (beam_cost == nullptr))
        return fail(GNNGLS_ERR_ARG, "beam_search: NULL pointer (beam_tours, beam_score and beam_cost are given together or not at all)");
    const int64_t need = (int64_t)gnngls::beam_workspace_bytes(B, n, width);
    if (!workspace || workspace_bytes < need)
        return fail(GNNGLS_ERR_ARG, "beam_search: workspace of %lld bytes is too small (gnngls_beam_search_workspace_bytes(%d, %d, %d) = "
                    "%lld)", workspace ? (long long)workspace_bytes : 0LL, B, n, width, (long long)need);
    if (((uintptr_t)workspace & 15u) != 0) return fail(GNNGLS_ERR_ARG, "beam_search: the workspace must be 16-byte aligned");
    hipError_t e = gnngls::launch_beam_search(S, D, B, n, width, depot, select, best_tour, best_score, best_cost, n_beams, status,
                                              beam_tours, beam_score, beam_cost, workspace, (hipStream_t)stream);
    return e == hipSuccess ? GNNGLS_OK : hip_fail(e, "beam_search");
}

static_assert(GNNGLS_GREEDY_EDGE_MAX_N == gnngls::kGreedyEdgeMaxN && GNNGLS_GREEDY_EDGE_BAD_SCORE == gnngls::kGreedyEdgeStatusBadScore &&
              GNNGLS_GREEDY_EDGE_STALLED == gnngls::kGreedyEdgeStatusStalled, "include/gnngls_hip.h and greedy_edge_kernels.h disagree");

int gnngls_greedy_edge(const double *S, const double *D, int B, int n, int depot, int32_t *tour, double *score, double *cost,
                       int32_t *edges, int32_t *rounds, int32_t *status, void *stream) {
    if (B < 1) return fail(GNNGLS_ERR_ARG, "greedy_edge: B=%d must be >= 1", B);
    if (n < 3) return fail(GNNGLS_ERR_ARG, "greedy_edge: n=%d must be >= 3", n);
    if (n > GNNGLS_GREEDY_EDGE_MAX_N)
        return fail(GNNGLS_ERR_ARG, "greedy_edge: n=%d exceeds the largest supported instance (n <= %d: one thread per node)", n,
                    GNNGLS_GREEDY_EDGE_MAX_N);
    if (depot < 0 || depot >= n) return fail(GNNGLS_ERR_ARG, "greedy_edge: depot=%d must be in [0, %d)", depot, n);
    if (!S || !tour || !score || !cost || !rounds || !status)
        return fail(GNNGLS_ERR_ARG, "greedy_edge: NULL pointer (S, tour, score, cost, rounds, status)");
    hipError_t e = gnngls::launch_greedy_edge(S, D, B, n, depot, tour, score, cost, edges, rounds, status, (hipStream_t)stream);
    return e == hipSuccess ? GNNGLS_OK : hip_fail(e, "greedy_edge");
}

int gnngls_gls_run(const double *D, const double *guides, int n_guides, int B, int n,
                   const int32_t *init_tour, const double *init_cost,
                   int perturbation_moves, int first_improvement, int penalty_bits,
                   int64_t max_outer_iters, double time_limit_s, double watchdog_s,
                   int32_t *best_tour, double *best_cost, int64_t *outer_iters,
                   double *trace_cost, float *trace_time, int trace_cap, int32_t *trace_len,
                   int32_t *penalty_out, int64_t *evals_out, int32_t *status,
                   double *imp_cost, float *imp_time, int64_t *imp_iter, int imp_cap, int32_t *imp_len, void *stream) {
    if (B == 0) return GNNGLS_OK;   // empty batch: nothing to enqueue (data pointers may be NULL)
    if (!D || !init_tour || !init_cost || !best_tour || !best_cost || B < 0 || n < 3 || n > 65535 || trace_cap < 0)
        return fail(GNNGLS_ERR_ARG, "gls_run: bad argument");
    if (imp_cap < 0 || ((imp_cost || imp_time || imp_iter) && !imp_len))
        return fail(GNNGLS_ERR_ARG, "gls_run: improvement trace needs imp_len and imp_cap >= 0");
    if (max_outer_iters != 0 && (!guides || n_guides < 1))
        return fail(GNNGLS_ERR_ARG, "gls_run: guides required when outer iterations are requested");
    if (!(watchdog_s > 0.0)) return fail(GNNGLS_ERR_ARG, "gls_run: watchdog_s must be > 0");
    if (!valid_penalty_bits(penalty_bits))
        return fail(GNNGLS_ERR_ARG, "gls_run: penalty_bits must be 0 (auto), 16, 32, -1 (global-memory store) or -2 (compact store)");
    hipStream_t st = (hipStream_t)stream;
    gnngls::GlsArgs A;
    memset(&A, 0, sizeof(A));
    A.D = D; A.guides = guides ? guides : D; A.n_guides = n_guides > 0 ? n_guides : 1; A.B = B; A.n = n;
    A.init_tour = init_tour; A.init_cost = init_cost;
    A.perturbation_moves = perturbation_moves;
    A.max_outer_iters = max_outer_iters; A.time_limit_s = time_limit_s; A.watchdog_s = watchdog_s;
    A.best_tour = best_tour; A.best_cost = best_cost; A.outer_iters = (long long *)outer_iters;
    A.trace_cost = trace_cost; A.trace_time = trace_time; A.trace_cap = trace_cost ? trace_cap : 0;
    A.pen16_limit = g_pen16_limit;
    A.imp_cost = imp_cost; A.imp_time = imp_time; A.imp_iter = (long long *)imp_iter; A.imp_cap = imp_cap; A.imp_len = imp_len;
    A.stamps = g_stamp_buffer;
    A.evals_exec = g_exec_evals.load(std::memory_order_relaxed);
    A.trace_len = trace_len; A.penalty_out = penalty_out; A.evals = (long long *)evals_out; A.status = status;
    const gnngls::GlsPlan cfg = plan_for(n, B, penalty_bits, first_improvement != 0, A.trace_cap > 0, A.evals_exec != nullptr);
    if (cfg.lds > kLdsPerCU)     // even the global-memory store keeps tours and per-position edge lengths in LDS
        return fail(GNNGLS_ERR_UNSUPPORTED, "gls_run: n=%d needs %zu B of LDS for tours and edge lengths (> 160 KiB)", n, cfg.lds);
    StreamScratch ws(st), asym(st), nl(st);      // freed behind the launch: neighbour lists, asymmetry flags, penalty workspace
    hipError_t e;
    if (cfg.store != gnngls::GLS_STORE_TRI) {
        // penalties in global memory (zeroed workspace): full matrices for the global store, packed
        // triangles for the compact store
        // global store: int32 [n,n] per instance; compact store: int32 packed triangle
        // (the team form of the compact store keeps a full symmetric matrix too: row-contiguous reads, see TriDGlobalPF)
        size_t per = (cfg.store == gnngls::GLS_STORE_GLOBAL || cfg.team) ? (size_t)n * n : (size_t)n * (n - 1) / 2;
        size_t bytes = (size_t)B * per * sizeof(int32_t);
        e = ws.alloc(bytes);
        if (e != hipSuccess) return hip_fail(e, "gls_run: workspace alloc");
        e = hipMemsetAsync(ws.p, 0, bytes, st);
        if (e != hipSuccess) return hip_fail(e, "gls_run: workspace memset");
        A.pen_ws = (int32_t *)ws.p;
    }
    if (A.evals_exec) {          // the wavefronts of an instance add their counts atomically
        // a run that prunes on an instantiation without the counting code cannot report the executed evaluations: -1
        e = hipMemsetAsync(A.evals_exec, 0, (size_t)GNNGLS_EXEC_RECORDS * B * sizeof(long long), st);       // counts + the cycle records
        if (e == hipSuccess && cfg.count_unknown) e = hipMemsetAsync(A.evals_exec, 0xff, (size_t)B * sizeof(long long), st);
        if (e != hipSuccess) return hip_fail(e, "gls_run: executed-evaluations buffer");
        if (cfg.count_unknown) A.evals_exec = nullptr;
    }
    // symmetric stores keep D[max, min] only: instances with an asymmetric matrix are flagged, not searched
    if (cfg.store != gnngls::GLS_STORE_GLOBAL) {
        e = asym.alloc((size_t)B * sizeof(int32_t));
        if (e == hipSuccess) e = gnngls::launch_symmetry_check(D, B, n, (int32_t *)asym.p, st);
        if (e != hipSuccess) return hip_fail(e, "gls_run: symmetry check");
        A.asym = (int32_t *)asym.p;
    }
    if (cfg.prune) {             // nearest-neighbour lists of the pruned descent scans
        const size_t entries = (size_t)B * n * gnngls::kNeighborListLen;
        e = nl.alloc((size_t)B * sizeof(int32_t) + entries);
        if (e != hipSuccess) return hip_fail(e, "gls_run: neighbour-list alloc");
        int32_t *ok = (int32_t *)nl.p;
        uint8_t *nl_id = (uint8_t *)(ok + B);
        e = gnngls::launch_neighbor_lists(D, B, n, nl_id, ok, st);
        if (e != hipSuccess) return hip_fail(e, "gls_run: neighbour lists");
        A.nl_id = nl_id; A.prune_ok = ok;
    }
    {
        ProfScope ps(GNNGLS_PROF_GLS, st);
        e = gnngls::launch_gls(A, cfg, st);
    }
    return e == hipSuccess ? GNNGLS_OK : hip_fail(e, "gls_run");
}

// ---- regret labels (datasets.py:23-34): chunks of fixed-edge jobs through gnngls_gls_run, see labels_kernels.h ----------------
int gnngls_regret_labels_chunk(int n) {
    if (n < 3 || n > 255) return 0;
    int J = gnngls_gls_resident_capacity(n);           // one resident workgroup per job
    if (J < 1) J = num_cus();
    const long cap = (512L << 20) / ((long)n * n * sizeof(double));      // D' of a chunk <= 512 MiB
    return (int)(J < cap ? J : cap);
}

int gnngls_regret_labels(const double *D, int B, int n, const int32_t *base_tour, const uint8_t *edge_mask,
                         int perturbation_moves, int64_t max_outer_iters, int penalty_bits, double watchdog_s, int chunk_jobs,
                         double *edge_cost, double *regret, int32_t *best_tour, double *best_cost, int32_t *status, void *stream) {
    if (B == 0) return GNNGLS_OK;   // empty batch: nothing to enqueue (data pointers may be NULL)
    if (!D || !base_tour || !edge_cost || !regret || !best_tour || !best_cost || !status || B < 0)
        return fail(GNNGLS_ERR_ARG, "regret_labels: bad argument (NULL pointer or B < 0)");
    if (n < 3 || n > 255) return fail(GNNGLS_ERR_ARG, "regret_labels: n=%d out of range (3..255)", n);
    if (max_outer_iters < 0)
        return fail(GNNGLS_ERR_ARG, "regret_labels: max_outer_iters must be >= 0 (labels are defined by an iteration count)");
    if (perturbation_moves < 0) return fail(GNNGLS_ERR_ARG, "regret_labels: perturbation_moves must be >= 0");
    if (!(watchdog_s > 0.0)) return fail(GNNGLS_ERR_ARG, "regret_labels: watchdog_s must be > 0");
    if (!valid_penalty_bits(penalty_bits))
        return fail(GNNGLS_ERR_ARG, "regret_labels: penalty_bits must be 0 (auto), 16, 32, -1 or -2");
    if (chunk_jobs < 0) return fail(GNNGLS_ERR_ARG, "regret_labels: chunk_jobs must be >= 0 (0 = gnngls_regret_labels_chunk(n))");
    hipStream_t st = (hipStream_t)stream;
    const int n1 = n + 1, N = n * (n - 1) / 2;
    // small per-instance workspace: M_b, base cost, rank of the best tour, asymmetry flags
    StreamScratch ws(st), cw(st);        // (the per-chunk workspace below: freed first)
    hipError_t e = ws.alloc((size_t)B * (3 * sizeof(double) + 2 * sizeof(int32_t)));
    if (e != hipSuccess) return hip_fail(e, "regret_labels: workspace alloc");
    double *offset = (double *)ws.p, *base_cost = offset + B;
    int32_t *best_rank = (int32_t *)(base_cost + 2 * B), *asym = best_rank + B;
    // the host builds the job lists: it needs the base tours (validated here) and the mask; an asymmetric D is rejected
    std::vector<int32_t> tours_h((size_t)B * n1), asym_h(B);
    std::vector<uint8_t> mask_h(edge_mask ? (size_t)B * N : 0);
    e = gnngls::launch_symmetry_check(D, B, n, asym, st);
    if (e == hipSuccess) e = hipMemcpyAsync(asym_h.data(), asym, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(tours_h.data(), base_tour, tours_h.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && edge_mask) e = hipMemcpyAsync(mask_h.data(), edge_mask, mask_h.size(), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return hip_fail(e, "regret_labels: reading the base tours");
    std::vector<int32_t> pos((size_t)B * n);
    for (int b = 0; b < B; ++b) {
        const int32_t *t = &tours_h[(size_t)b * n1];
        int32_t *pb = &pos[(size_t)b * n];
        for (int v = 0; v < n; ++v) pb[v] = -1;
        bool ok = t[0] == 0 && t[n] == 0;
        for (int p = 0; ok && p < n; ++p) {
            ok = t[p] >= 0 && t[p] < n && pb[t[p]] < 0;
            if (ok) pb[t[p]] = p;
        }
        if (!ok) return fail(GNNGLS_ERR_ARG, "regret_labels: base_tour[%d] is not a tour from depot 0", b);
        if (asym_h[b]) return fail(GNNGLS_ERR_ARG, "regret_labels: D[%d] is not symmetric (a fixed edge is an undirected edge)", b);
    }
    e = gnngls::launch_label_offsets(D, B, n, offset, st);
    if (e == hipSuccess) e = gnngls::launch_tour_cost(base_tour, D, B, n, base_cost, st);
    if (e == hipSuccess)
        e = gnngls::launch_label_init(B, n, base_tour, base_cost, edge_mask != nullptr, edge_cost, best_cost, best_rank, best_tour,
                                      status, st);
    if (e != hipSuccess) return hip_fail(e, "regret_labels: init");

    // per-chunk workspace: jobs, D' (= the guide), start and returned tours, costs, search status
    long total = 0;                                     // fixed-edge jobs of this call
    for (int b = 0; b < B; ++b) {
        const int32_t *pb = &pos[(size_t)b * n];
        for (int i = 0, r = 0; i < n; ++i)
            for (int j = i + 1; j < n; ++j, ++r) {
                const int gap = abs(pb[i] - pb[j]);
                total += gap != 1 && gap != n - 1 && (!edge_mask || mask_h[(size_t)b * N + r]);
            }
    }
    if (total == 0) {
        e = gnngls::launch_label_finalize(B, n, base_tour, base_cost, edge_cost, regret, st);
        return e == hipSuccess ? GNNGLS_OK : hip_fail(e, "regret_labels: finalize");
    }
    int J = chunk_jobs > 0 ? chunk_jobs : gnngls_regret_labels_chunk(n);
    if (J > total) J = (int)total;
    const size_t dp_bytes = (size_t)J * n * n * sizeof(double);
    const size_t cw_bytes = dp_bytes + (size_t)J * (sizeof(gnngls::LabelJob) + 2 * n1 * sizeof(int32_t) + 3 * sizeof(double) +
                                                    sizeof(int32_t));
    e = cw.alloc(cw_bytes);
    if (e != hipSuccess) return hip_fail(e, "regret_labels: chunk workspace alloc");
    double *Dp = (double *)cw.p, *init_cost = Dp + (size_t)J * n * n, *search_cost = init_cost + J, *job_cost = search_cost + J;
    gnngls::LabelJob *jobs_d = (gnngls::LabelJob *)(job_cost + J);
    int32_t *tin = (int32_t *)(jobs_d + J), *tout = tin + (size_t)J * n1, *job_status = tout + (size_t)J * n1;

    // one chunk: expand, search, collect; then (16-bit counters) rerun the jobs that overflowed with 32-bit counters
    std::vector<int32_t> status_h(J);
    std::function<int(const std::vector<gnngls::LabelJob> &, int)> run = [&](const std::vector<gnngls::LabelJob> &jobs, int bits) {
        const int cnt = (int)jobs.size();
        hipError_t he = hipMemcpyAsync(jobs_d, jobs.data(), (size_t)cnt * sizeof(gnngls::LabelJob), hipMemcpyHostToDevice, st);
        if (he == hipSuccess) he = gnngls::launch_label_expand(D, n, base_tour, jobs_d, cnt, offset, Dp, tin, st);
        if (he == hipSuccess) he = gnngls::launch_tour_cost(tin, Dp, cnt, n, init_cost, st);
        if (he != hipSuccess) return hip_fail(he, "regret_labels: expansion");
        const int rc = gnngls_gls_run(Dp, Dp, 1, cnt, n, tin, init_cost, perturbation_moves, 0, bits, max_outer_iters, 0.0, watchdog_s,
                                      tout, search_cost, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, job_status,
                                      nullptr, nullptr, nullptr, 0, nullptr, stream);
        if (rc != GNNGLS_OK) return rc;
        he = gnngls::launch_label_collect(D, n, jobs_d, cnt, tout, job_status, job_cost, edge_cost, best_cost, best_rank, best_tour,
                                          status, st);
        if (he == hipSuccess) he = hipMemcpyAsync(status_h.data(), job_status, (size_t)cnt * sizeof(int32_t), hipMemcpyDeviceToHost, st);
        if (he == hipSuccess) he = hipStreamSynchronize(st);      // (also: the host job list may be reused)
        if (he != hipSuccess) return hip_fail(he, "regret_labels: labels");
        std::vector<gnngls::LabelJob> again;
        for (int k = 0; k < cnt; ++k)
            if (status_h[k] == GNNGLS_STATUS_PENALTY_OVERFLOW) again.push_back(jobs[k]);
        if (again.empty()) return (int)GNNGLS_OK;
        if (bits != 0 && bits != 16) return fail(GNNGLS_ERR_HIP, "regret_labels: penalty overflow with %d-bit counters", bits);
        return run(again, 32);
    };
    std::vector<gnngls::LabelJob> chunk;
    chunk.reserve(J);
    for (int b = 0; b < B; ++b) {
        const int32_t *pb = &pos[(size_t)b * n];
        for (int i = 0, r = 0; i < n; ++i)
            for (int j = i + 1; j < n; ++j, ++r) {
                const int gap = abs(pb[i] - pb[j]);
                if (gap == 1 || gap == n - 1) continue;                 // on the base tour: regret 0
                if (edge_mask && !mask_h[(size_t)b * N + r]) continue;  // kept from an earlier call
                chunk.push_back(gnngls::LabelJob{b, i, j, r});
                if ((int)chunk.size() == J) {
                    const int rc = run(chunk, penalty_bits);
                    if (rc != GNNGLS_OK) return rc;
                    chunk.clear();
                }
            }
    }
    if (!chunk.empty()) {
        const int rc = run(chunk, penalty_bits);
        if (rc != GNNGLS_OK) return rc;
    }
    e = gnngls::launch_label_finalize(B, n, base_tour, base_cost, edge_cost, regret, st);
    return e == hipSuccess ? GNNGLS_OK : hip_fail(e, "regret_labels: finalize");
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------
// GNN forward
// ---------------------------------------------------------------------------------------------
namespace {
// the parameters of one layer inside the packed weights (and, with T = float, of their gradients)
template <typename T>
struct LayerParams { T *fc_w, *attn_l, *attn_r, *bn1_g, *bn1_b, *w1, *b1, *w2, *b2, *bn2_g, *bn2_b; };
template <typename T>
LayerParams<T> layer_params(T *w, const gnngls::PackedModel &m, int l) {
    const gnngls::LayerOffsets o = m.layer(l);
    return {w + o.fc_w, w + o.attn_l, w + o.attn_r, w + o.bn1_g, w + o.bn1_b, w + o.w1, w + o.b1, w + o.w2, w + o.b2, w + o.bn2_g, w + o.bn2_b};
}
#define GNNGLS_TRY(x) do { e = (x); if (e != hipSuccess) return hip_fail(e, #x); } while (0)

// the experiment switches (A/B runs), read once per process: the only place of the model's code that looks at the environment
const gnngls::ForwardSwitches &forward_switches() {
    static const gnngls::ForwardSwitches sw = [] {
        gnngls::ForwardSwitches v;
        const char *fp32 = getenv("GNNGLS_FFN_FP32"), *rank1 = getenv("GNNGLS_GAT_RANK1"), *heads = getenv("GNNGLS_GAT_HEADS");
        v.ffn_fp32 = fp32 && atoi(fp32) != 0;
        v.rank1_mode = rank1 && atoi(rank1) == 0 ? 0 : rank1 && atoi(rank1) == 2 ? 2 : -1;
        v.gat_heads = !heads ? 0 : atoi(heads) == 4 ? 4 : 8;       // (set to anything but 4: the unsplit form)
        return v;
    }();
    return sw;
}

int heads_fail(const char *what, int n_heads) {
    return fail(GNNGLS_ERR_UNSUPPORTED, "%s: n_heads=%d is not supported (embed_dim 128: n_heads in {1, 2, 4, 8, 16})", what, n_heads);
}

unsigned char *align256(const void *p) { return (unsigned char *)(((uintptr_t)p + 255) & ~(uintptr_t)255); }
}  // namespace

extern "C" {

int64_t gnngls_model_packed_floats(int in_dim, int n_layers) {
    if (in_dim < 0 || n_layers < 0) return 0;
    return gnngls::packed_model(in_dim, n_layers).total;
}

int64_t gnngls_regret_forward_workspace_bytes(int B, int n) { return gnngls_regret_forward_workspace_bytes_heads(B, n, 8); }

int64_t gnngls_regret_prepared_bytes(int n_layers) {
    if (n_layers < 0) return 0;
    return (int64_t)gnngls::prepared_bytes(n_layers);
}

int gnngls_regret_prepare(const float *weights, int in_dim, int n_layers, void *prepared, int64_t prepared_bytes, void *stream) {
    if (!weights || !prepared || in_dim < 1 || n_layers < 0) return fail(GNNGLS_ERR_ARG, "regret_prepare: bad argument");
    if (prepared_bytes < gnngls_regret_prepared_bytes(n_layers))
        return fail(GNNGLS_ERR_ARG, "regret_prepare: buffer too small (%lld B, need %lld B)", (long long)prepared_bytes,
                    (long long)gnngls_regret_prepared_bytes(n_layers));
    unsigned char *base = align256(prepared);
    const gnngls::PackedModel m = gnngls::packed_model(in_dim, n_layers);
    for (int l = 0; l < n_layers; ++l) {
        const LayerParams<const float> p = layer_params(weights, m, l);
        const float *fc_next = l + 1 < n_layers ? weights + m.layer(l + 1).fc_w : nullptr;
        hipError_t e = gnngls::launch_ffn_pack(p.w1, p.w2, fc_next, base + gnngls::prepared_layer(l), (hipStream_t)stream);
        if (e != hipSuccess) return hip_fail(e, "regret_prepare");
    }
    if (n_layers > 0 && in_dim <= gnngls::kEmbedFcMaxIn) {
        const LayerParams<const float> p = layer_params(weights, m, 0);
        hipError_t e = gnngls::launch_embed_fc_prepare(weights + m.emb_w, weights + m.emb_b, p.fc_w, p.attn_l, p.attn_r, in_dim,
                                                       base + gnngls::prepared_embed_fc(n_layers), (hipStream_t)stream);
        if (e != hipSuccess) return hip_fail(e, "regret_prepare");
    }
    return GNNGLS_OK;
}

}  // extern "C"

namespace {
// the attention of one layer as the plan (of the forward or of the training step) shaped it
hipError_t launch_attention(const gnngls::AttnStep &a, const float *ft, const float *attn_l, const float *attn_r, int B, int n,
                            float *part, float *part_ms, float *hms, hipStream_t st) {
    if (a.form == gnngls::ATTN_K1) return gnngls::launch_gat_rows(ft, attn_l, attn_r, B, n, a.heads_per_wg, a.waves, part, part_ms, st);
    return gnngls::launch_gat_heads_rows(ft, attn_l, attn_r, B, n, gnngls::kD / a.F, a.waves, part, part_ms, hms, st);
}

// Every forward entry point: makes the request, takes the plan (model_plan.cpp), and executes its steps chunk by chunk.
// one_call: no image from the caller -- the weights are split into stream-ordered scratch of this call (gnngls_regret_prepare +
// gnngls_regret_forward_prepared keep the image across calls: 2 launches per layer and the allocation saved per forward).
int run_forward(bool one_call, const float *feat, const float *weights, const void *prepared, int64_t prepared_bytes, int B, int n,
                int in_dim, int n_layers, int n_heads, float *y_out, void *workspace, int64_t workspace_bytes, void *stream) {
    unsigned char *base = align256(workspace);
    const gnngls::ForwardPlan plan = gnngls::forward_plan({n, B, in_dim, n_layers, n_heads, feat && weights && y_out && workspace, one_call,
                                                           prepared != nullptr, prepared_bytes,
                                                           workspace_bytes - (int64_t)(base - (unsigned char *)workspace), forward_switches()});
    hipStream_t st = (hipStream_t)stream;
    StreamScratch scratch(st);
    if (plan.build_image) {
        prepared_bytes = gnngls_regret_prepared_bytes(n_layers);
        hipError_t e = scratch.alloc((size_t)prepared_bytes);
        if (e != hipSuccess) return hip_fail(e, "regret_forward: scratch alloc");
        const int rc = gnngls_regret_prepare(weights, in_dim, n_layers, scratch.p, prepared_bytes, stream);
        if (rc != GNNGLS_OK) return rc;
        prepared = scratch.p;
    }
    switch (plan.why) {
    case gnngls::FWD_OK: break;
    case gnngls::FWD_BAD_HEADS: return heads_fail("regret_forward", n_heads);
    case gnngls::FWD_BAD_ARG: return fail(plan.status, "regret_forward: bad argument");
    case gnngls::FWD_K1_LDS:
        return fail(plan.status, "regret_forward: n=%d needs %zu B of LDS per row tile (> 160 KiB)", n, (size_t)plan.number);
    case gnngls::FWD_K1H_NODES:
        return fail(plan.status, "regret_forward: n=%d exceeds the %d-head attention tile limit (n <= %d; 8 heads: n <= 423)", n, n_heads,
                    (int)plan.number);
    case gnngls::FWD_IMAGE_SMALL:
        return fail(plan.status, "regret_forward: prepared image too small (%lld B, need %lld B)", (long long)prepared_bytes,
                    (long long)plan.number);
    case gnngls::FWD_WORKSPACE_SMALL:
        return fail(plan.status, "regret_forward: workspace too small (%lld B, need >= %lld B)", (long long)workspace_bytes,
                    (long long)plan.number);
    }
    if (plan.Bc == 0) return GNNGLS_OK;   // empty batch: nothing to enqueue (data pointers may be NULL)
    const gnngls::PackedModel m = gnngls::packed_model(in_dim, n_layers);
    const unsigned char *image = plan.use_image ? align256(prepared) : nullptr;
    const float *img0 = (const float *)(image ? image + gnngls::prepared_embed_fc(n_layers) : nullptr);      // the embed-fc image
    const long N = (long)n * (n - 1) / 2;
    float *h = (float *)(base + plan.ws.h), *ft = (float *)(base + plan.ws.ft), *part = (float *)(base + plan.ws.part);
    float *part_ms = (float *)(base + plan.ws.part_ms), *h2 = (float *)(base + plan.ws.h2), *hms = (float *)(base + plan.ws.hms);
    const float *emb_w = weights + m.emb_w, *emb_b = weights + m.emb_b, *dec_w = weights + m.dec_w, *dec_b = weights + m.dec_b;
    hipError_t e = hipSuccess;
    for (long b0 = 0; b0 < B; b0 += plan.Bc) {
        const int bc = (int)((B - b0) < plan.Bc ? (B - b0) : plan.Bc);
        const long M = (long)bc * N;
        const float *x = feat + b0 * N * in_dim;
        if (plan.embed != gnngls::EMBED_NONE) {                                                       // models.py:66
          ProfScope ps(GNNGLS_PROF_EMBED, st);
          if (plan.embed == gnngls::EMBED_PLAIN) GNNGLS_TRY(gnngls::launch_embed(x, emb_w, emb_b, h, M, in_dim, st));
          else GNNGLS_TRY(gnngls::launch_embed_fc(x, emb_w, emb_b, img0, h, plan.embed == gnngls::EMBED_FC ? ft : nullptr, M, in_dim, st)); }
        for (int l = 0; l < n_layers; ++l) {                                                          // models.py:67-68
            const gnngls::LayerStep &step = plan.layer(l);
            const LayerParams<const float> p = layer_params(weights, m, l);
            if (step.fc_launch) {                                                                     // ft = fc(h), models.py:23
              ProfScope ps(GNNGLS_PROF_GEMM_FC, st);
              GNNGLS_TRY(gnngls::launch_gemm(gnngls::GEMM_EPI_STORE, h, p.fc_w, ft, M, 128, 128, nullptr, nullptr, nullptr, nullptr, st)); }
            switch (step.attn.form) {
            case gnngls::ATTN_RANK1: case gnngls::ATTN_RANK1_COMPACT: {
              ProfScope ps(GNNGLS_PROF_GAT_ROWS_RANK1, st);
              GNNGLS_TRY(gnngls::launch_gat_rows_rank1(x, img0, bc, n, part, part_ms, st, step.attn.form == gnngls::ATTN_RANK1_COMPACT));
              break; }
            case gnngls::ATTN_K1: case gnngls::ATTN_K1H: {
              ProfScope ps(GNNGLS_PROF_GAT_ROWS, st);
              GNNGLS_TRY(launch_attention(step.attn, ft, p.attn_l, p.attn_r, bc, n, part, part_ms, hms, st));
              if (step.attn.merge16) GNNGLS_TRY(gnngls::launch_gat_heads_merge16(part, hms, part_ms, M, st));
              break; }
            }
            // gat_combine + FFN1 + FFN2 in one launch; the hidden layer and x = BN1(h + GAT) never touch HBM
            { ProfScope ps(GNNGLS_PROF_FFN_FUSED, st);
              const gnngls::FfnFused a = {part, part_ms, step.ffn.rank1_input ? x : h, p.bn1_g, p.bn1_b, p.w1, p.b1, p.w2, p.b2, p.bn2_g, p.bn2_b,
                                          h2, M, image ? image + gnngls::prepared_layer(l) : nullptr, ft, dec_w, dec_b, y_out + b0 * N, img0, emb_w, emb_b};
              GNNGLS_TRY(gnngls::launch_ffn_fused(a, step.ffn, st)); }
            { float *t = h; h = h2; h2 = t; }
        }
        if (plan.decision_launch) {                                                                   // models.py:69
          ProfScope ps(GNNGLS_PROF_DECISION, st);
          GNNGLS_TRY(gnngls::launch_decision(h, dec_w, dec_b, y_out + b0 * N, M, st)); }
    }
    return GNNGLS_OK;
}
}  // namespace

extern "C" {

int gnngls_regret_forward_prepared(const float *feat, const float *weights, const void *prepared, int64_t prepared_bytes,
                                   int B, int n, int in_dim, int n_layers,
                                   float *y_out, void *workspace, int64_t workspace_bytes, void *stream) {
    return run_forward(false, feat, weights, prepared, prepared_bytes, B, n, in_dim, n_layers, 8, y_out, workspace, workspace_bytes, stream);
}

int gnngls_regret_forward(const float *feat, const float *weights, int B, int n, int in_dim, int n_layers,
                          float *y_out, void *workspace, int64_t workspace_bytes, void *stream) {
    return run_forward(true, feat, weights, nullptr, 0, B, n, in_dim, n_layers, 8, y_out, workspace, workspace_bytes, stream);
}

// ---- head counts other than 8 (embed_dim 128): the same forward with the attention of heads_kernels.hip ----------------------
int gnngls_model_heads_supported(int n_heads) { return gnngls::heads_supported(n_heads) ? 1 : 0; }

int64_t gnngls_regret_forward_workspace_bytes_heads(int B, int n, int n_heads) {
    if (!gnngls::heads_supported(n_heads)) return 0;
    if (B < 1 || n < 2 || n > 65535) return 0;          // 65535 nodes x 2^31 instances still fits an int64
    return (int64_t)gnngls::forward_layout((long)B * ((long)n * (n - 1) / 2), n_heads).end + 256;
}

int gnngls_regret_prepare_heads(const float *weights, int in_dim, int n_layers, int n_heads, void *prepared, int64_t prepared_bytes,
                                void *stream) {
    if (!gnngls::heads_supported(n_heads)) return heads_fail("regret_prepare", n_heads);
    // (the image does not depend on the head count: its rank-1 first-layer coefficients are only read by the 8-head forward)
    return gnngls_regret_prepare(weights, in_dim, n_layers, prepared, prepared_bytes, stream);
}

int gnngls_regret_forward_prepared_heads(const float *feat, const float *weights, const void *prepared, int64_t prepared_bytes,
                                         int B, int n, int in_dim, int n_layers, int n_heads,
                                         float *y_out, void *workspace, int64_t workspace_bytes, void *stream) {
    return run_forward(false, feat, weights, prepared, prepared_bytes, B, n, in_dim, n_layers, n_heads, y_out, workspace, workspace_bytes,
                       stream);
}

int gnngls_regret_forward_heads(const float *feat, const float *weights, int B, int n, int in_dim, int n_layers, int n_heads,
                                float *y_out, void *workspace, int64_t workspace_bytes, void *stream) {
    return run_forward(true, feat, weights, nullptr, 0, B, n, in_dim, n_layers, n_heads, y_out, workspace, workspace_bytes, stream);
}

int gnngls_pack_features(const double *D, int B, int n, double scale, double min_, float *feat, void *stream) {
    if (B == 0) return GNNGLS_OK;   // empty batch: nothing to enqueue (data pointers may be NULL)
    if (!D || !feat || B < 0 || n < 2) return fail(GNNGLS_ERR_ARG, "pack_features: bad argument");
    ProfScope ps(GNNGLS_PROF_PACK, (hipStream_t)stream);
    hipError_t e = gnngls::launch_pack_features(D, B, n, scale, min_, feat, (hipStream_t)stream);
    return e == hipSuccess ? GNNGLS_OK : hip_fail(e, "pack_features");
}

int gnngls_unpack_regret(const float *y, int B, int n, double scale, double min_, double *out, void *stream) {
    if (B == 0) return GNNGLS_OK;   // empty batch: nothing to enqueue (data pointers may be NULL)
    if (!y || !out || B < 0 || n < 2) return fail(GNNGLS_ERR_ARG, "unpack_regret: bad argument");
    ProfScope ps(GNNGLS_PROF_UNPACK, (hipStream_t)stream);
    hipError_t e = gnngls::launch_unpack_regret(y, B, n, scale, min_, out, (hipStream_t)stream);
    return e == hipSuccess ? GNNGLS_OK : hip_fail(e, "unpack_regret");
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------
// GNN training step (forward with batch-statistics BatchNorm + backward)
// ---------------------------------------------------------------------------------------------
namespace {

// Both halves of the step: makes the request, takes the plan (model_plan.cpp: the refusals, the workspace layout, the attention
// forms of both ways) and prints its refusal.  io: y_out / grads.
int train_begin(const char *what, const void *feat, const void *params, const void *io, const void *workspace, int B, int n, int in_dim,
                int n_layers, int n_heads, int64_t workspace_bytes, gnngls::TrainPlan &plan) {
    plan = gnngls::train_plan({n, B, in_dim, n_layers, n_heads, feat && params && io && workspace, workspace_bytes,
                               forward_switches().gat_heads});
    switch (plan.why) {
    case gnngls::TRAIN_OK: break;
    case gnngls::TRAIN_BAD_HEADS: return heads_fail(what, n_heads);
    case gnngls::TRAIN_BAD_ARG: return fail(plan.status, "%s: bad argument", what);
    case gnngls::TRAIN_BWD_NODES:
        return fail(plan.status, "%s: n=%d exceeds the attention-backward tile limit (n <= %d)", what, n, (int)plan.number);
    case gnngls::TRAIN_WORKSPACE_SMALL:
        return fail(plan.status, "%s: workspace too small (%lld B, need %lld B)", what, (long long)workspace_bytes, (long long)plan.number);
    }
    return GNNGLS_OK;
}

// the attention backward of one layer as the plan shaped it ...
hipError_t launch_attention_bwd(const gnngls::AttnBwdStep &a, const float *ft, const float *dout, const float *gout, const float *att,
                                const float *attn_l, const float *attn_r, int B, int n, float *P, float *dlr, hipStream_t st) {
    if (a.form == gnngls::ATTN_K1) return gnngls::launch_gat_bwd_rows(ft, dout, gout, att, attn_l, attn_r, B, n, a.tiles, a.lds, P, dlr, st);
    return gnngls::launch_gat_heads_bwd_rows(ft, dout, gout, att, attn_l, attn_r, B, n, gnngls::kD / a.F, a.lds, P, dlr, st);
}

// ... and its combine: dft = P + del * attn_l + der * attn_r, d el / d er per slot or (16 heads) per head
hipError_t launch_attention_bwd_combine(gnngls::CombineForm form, const float *P, const float *dlr, const float *attn_l, const float *attn_r,
                                        long M, float *dft, float *dl, float *dr, hipStream_t st) {
    if (form == gnngls::COMBINE_HEADS16) return gnngls::launch_gat_heads_bwd_combine16(P, dlr, attn_l, attn_r, M, dft, dl, dr, st);
    return gnngls::launch_gat_bwd_combine(P, dlr, attn_l, attn_r, M, dft, dl, dr, st);
}

}  // namespace

extern "C" {

int64_t gnngls_regret_train_workspace_bytes(int B, int n, int n_layers) { return gnngls_regret_train_workspace_bytes_heads(B, n, n_layers, 8); }

int64_t gnngls_regret_train_workspace_bytes_heads(int B, int n, int n_layers, int n_heads) {
    return gnngls::train_workspace_bytes(B, n, n_layers, n_heads);
}

int gnngls_regret_train_forward(const float *feat, const float *params, int B, int n, int in_dim, int n_layers, float bn_eps,
                                float *y_out, float *bn_batch_stats, void *workspace, int64_t workspace_bytes, void *stream) {
    return gnngls_regret_train_forward_heads(feat, params, B, n, in_dim, n_layers, 8, bn_eps, y_out, bn_batch_stats, workspace,
                                             workspace_bytes, stream);
}

int gnngls_regret_train_forward_heads(const float *feat, const float *params, int B, int n, int in_dim, int n_layers, int n_heads,
                                      float bn_eps, float *y_out, float *bn_batch_stats, void *workspace, int64_t workspace_bytes,
                                      void *stream) {
    gnngls::TrainPlan plan;
    int rc = train_begin("regret_train_forward", feat, params, y_out, workspace, B, n, in_dim, n_layers, n_heads, workspace_bytes, plan);
    if (rc != GNNGLS_OK) return rc;
    if (!bn_batch_stats && n_layers > 0) return fail(GNNGLS_ERR_ARG, "regret_train_forward: bn_batch_stats is NULL");
    hipStream_t st = (hipStream_t)stream;
    const gnngls::TrainLayout &w = plan.ws;
    const long M = w.M;
    unsigned char *base = align256(workspace);
    auto at = [base](size_t offset) { return (float *)(base + offset); };
    const gnngls::PackedModel m = gnngls::packed_model(in_dim, n_layers);
    float *part = at(w.PART), *pms = at(w.PMS), *ones = at(w.ONES), *zeros = at(w.ZEROS);
    double *csp = (double *)(base + w.CSP);
    hipError_t e = hipSuccess;
    const float one = 1.f;
    uint32_t one_bits;
    memcpy(&one_bits, &one, 4);
    GNNGLS_TRY(hipMemsetD32Async((hipDeviceptr_t)ones, (int)one_bits, 128, st));
    GNNGLS_TRY(hipMemsetAsync(zeros, 0, 512 * sizeof(float), st));
    { ProfScope ps(GNNGLS_PROF_EMBED, st);
      GNNGLS_TRY(gnngls::launch_embed(feat, params + m.emb_w, params + m.emb_b, at(w.h(0)), M, in_dim, st)); }                 // models.py:66
    for (int l = 0; l < n_layers; ++l) {                                                                // models.py:67-68
        const LayerParams<const float> p = layer_params(params, m, l);
        const float *h = at(w.h(l));
        float *ft = at(w.ft(l)), *g = at(w.g(l)), *h1 = at(w.h1(l)), *h3 = at(w.h3(l)), *att = at(w.att(l));
        float *scale1 = at(w.bn(l, gnngls::BN_SCALE1)), *shift1 = at(w.bn(l, gnngls::BN_SHIFT1));
        float *scale2 = at(w.bn(l, gnngls::BN_SCALE2)), *shift2 = at(w.bn(l, gnngls::BN_SHIFT2));
        int nb = 0;
        { ProfScope ps(GNNGLS_PROF_GEMM_FC, st);
          GNNGLS_TRY(gnngls::launch_gemm(gnngls::GEMM_EPI_STORE, h, p.fc_w, ft, M, 128, 128, nullptr, nullptr, nullptr, nullptr, st)); }
        // (16 heads: the per-head statistics of the forward kernel go where the slot statistics go otherwise, into the widened PMS)
        { ProfScope ps(GNNGLS_PROF_GAT_ROWS, st);
          GNNGLS_TRY(launch_attention(plan.attn, ft, p.attn_l, p.attn_r, B, n, part, pms, pms, st)); }
        // (H <= 8: slot statistics, gat_combine_train_kernel, models.py:12-15; H = 16: per-head statistics and their own merge)
        { ProfScope ps(GNNGLS_PROF_TRAIN_ELEMENTWISE, st);
          if (plan.combine == gnngls::COMBINE_HEADS16) GNNGLS_TRY(gnngls::launch_gat_heads_merge16_train(part, pms, h, M, g, h1, att, st));
          else GNNGLS_TRY(gnngls::launch_gat_combine_train(part, pms, h, M, g, h1, att, st)); }
        { ProfScope ps(GNNGLS_PROF_TRAIN_COLSUM, st);                                                   // models.py:27 (train mode)
          GNNGLS_TRY(gnngls::launch_colsum(gnngls::CS_SUM_SQ, h1, nullptr, nullptr, M, 128, 0, csp, &nb, st));
          GNNGLS_TRY(gnngls::launch_bn_stats_finalize(csp, nb, M, p.bn1_g, p.bn1_b, bn_eps, scale1, shift1, at(w.bn(l, gnngls::BN_MEAN1)),
                                                      at(w.bn(l, gnngls::BN_INVSTD1)), bn_batch_stats + gnngls::batch_stat(l, gnngls::STAT_MEAN1),
                                                      bn_batch_stats + gnngls::batch_stat(l, gnngls::STAT_VAR1), st)); }
        { ProfScope ps(GNNGLS_PROF_FFN_FUSED, st);                                                      // models.py:28-33
          GNNGLS_TRY(gnngls::launch_ffn_fused_train(h1, scale1, shift1, p.w1, p.b1, p.w2, p.b2, ones, zeros, h3, at(w.hid(l)), M, st)); }
        { ProfScope ps(GNNGLS_PROF_TRAIN_COLSUM, st);                                                   // models.py:35 (train mode)
          GNNGLS_TRY(gnngls::launch_colsum(gnngls::CS_SUM_SQ, h3, nullptr, nullptr, M, 128, 0, csp, &nb, st));
          GNNGLS_TRY(gnngls::launch_bn_stats_finalize(csp, nb, M, p.bn2_g, p.bn2_b, bn_eps, scale2, shift2, at(w.bn(l, gnngls::BN_MEAN2)),
                                                      at(w.bn(l, gnngls::BN_INVSTD2)), bn_batch_stats + gnngls::batch_stat(l, gnngls::STAT_MEAN2),
                                                      bn_batch_stats + gnngls::batch_stat(l, gnngls::STAT_VAR2), st)); }
        { ProfScope ps(GNNGLS_PROF_TRAIN_ELEMENTWISE, st);
          GNNGLS_TRY(gnngls::launch_affine_cols(h3, scale2, shift2, at(w.h(l + 1)), M, st)); }
    }
    { ProfScope ps(GNNGLS_PROF_DECISION, st);
      GNNGLS_TRY(gnngls::launch_decision(at(w.h(n_layers)), params + m.dec_w, params + m.dec_b, y_out, M, st)); }             // models.py:69
    return GNNGLS_OK;
}

int gnngls_regret_train_backward(const float *feat, const float *params, const float *dy, int B, int n, int in_dim,
                                 int n_layers, float *grads, void *workspace, int64_t workspace_bytes, void *stream) {
    return gnngls_regret_train_backward_heads(feat, params, dy, B, n, in_dim, n_layers, 8, grads, workspace, workspace_bytes, stream);
}

int gnngls_regret_train_backward_heads(const float *feat, const float *params, const float *dy, int B, int n, int in_dim,
                                       int n_layers, int n_heads, float *grads, void *workspace, int64_t workspace_bytes,
                                       void *stream) {
    gnngls::TrainPlan plan;
    int rc = train_begin("regret_train_backward", feat, params, grads, workspace, B, n, in_dim, n_layers, n_heads, workspace_bytes, plan);
    if (rc != GNNGLS_OK) return rc;
    if (!dy) return fail(GNNGLS_ERR_ARG, "regret_train_backward: dy is NULL");
    hipStream_t st = (hipStream_t)stream;
    const gnngls::TrainLayout &w = plan.ws;
    const long M = w.M;
    unsigned char *base = align256(workspace);
    auto at = [base](size_t offset) { return (float *)(base + offset); };
    const gnngls::PackedModel m = gnngls::packed_model(in_dim, n_layers);       // the parameters and, same layout, their gradients
    const float *dec_w = params + m.dec_w;
    float *g_emb_w = grads + m.emb_w, *g_emb_b = grads + m.emb_b, *g_dec_w = grads + m.dec_w, *g_dec_b = grads + m.dec_b;
    float *part = at(w.PART), *pms = at(w.PMS), *da = at(w.DA), *db = at(w.DB), *x2 = at(w.X2), *dft = at(w.DFT), *dl = at(w.DL), *dr = at(w.DR);
    float *w2t = at(w.W2T), *w1t = at(w.W1T), *coef = at(w.COEF), *tnp = at(w.TNP);
    double *csp = (double *)(base + w.CSP);
    hipError_t e = hipSuccess;
    int nb = 0;
    GNNGLS_TRY(hipMemsetAsync(g_dec_b + 1, 0, 3 * sizeof(float), st));                                   // pad
    // decision layer (models.py:69): y = h.w + b
    { ProfScope ps(GNNGLS_PROF_TRAIN_COLSUM, st);
      GNNGLS_TRY(gnngls::launch_colsum(gnngls::CS_ROWSCALE, at(w.h(n_layers)), dy, nullptr, M, 128, 1, csp, &nb, st));
      GNNGLS_TRY(gnngls::launch_colsum_store(csp, nb, 128, 1, g_dec_w, nullptr, st));
      GNNGLS_TRY(gnngls::launch_sum_vector(dy, M, g_dec_b, st)); }
    { ProfScope ps(GNNGLS_PROF_TRAIN_ELEMENTWISE, st);
      GNNGLS_TRY(gnngls::launch_outer_rows(dy, dec_w, da, M, st)); }
    for (int l = n_layers - 1; l >= 0; --l) {
        const LayerParams<const float> p = layer_params(params, m, l);
        const LayerParams<float> d = layer_params(grads, m, l);
        const float *h = at(w.h(l)), *ft = at(w.ft(l)), *g = at(w.g(l)), *h1 = at(w.h1(l)), *h3 = at(w.h3(l)), *att = at(w.att(l));
        const float *mean1 = at(w.bn(l, gnngls::BN_MEAN1)), *invstd1 = at(w.bn(l, gnngls::BN_INVSTD1));
        const float *mean2 = at(w.bn(l, gnngls::BN_MEAN2)), *invstd2 = at(w.bn(l, gnngls::BN_INVSTD2));
        // BatchNorm 2 backward (models.py:35): DA = d(layer output) -> DB = d h3
        { ProfScope ps(GNNGLS_PROF_TRAIN_COLSUM, st);
          GNNGLS_TRY(gnngls::launch_colsum(gnngls::CS_SUM_PROD, da, h3, nullptr, M, 128, 0, csp, &nb, st));
          GNNGLS_TRY(gnngls::launch_bn_bwd_finalize(csp, nb, M, p.bn2_g, mean2, invstd2, d.bn2_g, d.bn2_b, coef, st)); }
        { ProfScope ps(GNNGLS_PROF_TRAIN_ELEMENTWISE, st);
          // d h3 = BatchNorm-2 backward of DA, and x = BN1(h1) recomputed, in one elementwise pass
          GNNGLS_TRY(gnngls::launch_bn_bwd_apply_and_affine(da, h3, mean2, coef, db, h1, at(w.bn(l, gnngls::BN_SCALE1)),
                                                            at(w.bn(l, gnngls::BN_SHIFT1)), x2, M, st));
          GNNGLS_TRY(gnngls::launch_transpose_pair(p.w2, p.w1, w2t, w1t, st)); }                             // W2^T, W1^T
        // feed-forward block backward (models.py:28-33): h3 = x + W2 relu(W1 x + b1) + b2
        float *hid = at(w.hid(l));                           // saved ReLU(W1 x + b1)
        { ProfScope ps(GNNGLS_PROF_TRAIN_GEMM_TN, st);
          GNNGLS_TRY(gnngls::launch_gemm_tn(db, hid, M, 128, 512, tnp, d.w2, d.b2, st)); }       // d W2 and d b2 = colsum(d h3)
        { ProfScope ps(GNNGLS_PROF_TRAIN_GEMM_BWD, st);      // d x = ((d h3 * W2) . [relu > 0]) * W1 + d h3; hid <- d pre
          GNNGLS_TRY(gnngls::launch_ffn_fused_bwd(db, w2t, w1t, at(w.ONES), at(w.ZEROS), da, hid, M, st)); }
        { ProfScope ps(GNNGLS_PROF_TRAIN_GEMM_TN, st);
          GNNGLS_TRY(gnngls::launch_gemm_tn(hid, x2, M, 512, 128, tnp, d.w1, d.b1, st)); }       // d W1 and d b1 = colsum(d pre)
        // BatchNorm 1 backward (models.py:27): DA = d x -> DB = d h1 (= d h through the skip, = d GATConv output)
        { ProfScope ps(GNNGLS_PROF_TRAIN_COLSUM, st);
          GNNGLS_TRY(gnngls::launch_colsum(gnngls::CS_SUM_PROD, da, h1, nullptr, M, 128, 0, csp, &nb, st));
          GNNGLS_TRY(gnngls::launch_bn_bwd_finalize(csp, nb, M, p.bn1_g, mean1, invstd1, d.bn1_g, d.bn1_b, coef, st)); }
        { ProfScope ps(GNNGLS_PROF_TRAIN_ELEMENTWISE, st);
          GNNGLS_TRY(gnngls::launch_bn_bwd_apply(da, h1, mean1, coef, db, M, st)); }
        // GATConv backward (models.py:23): attention backward, combine, the attn_l / attn_r column sums (d el / d er per slot, or
        // with 16 heads per head: combine and sums of their own)
        { ProfScope ps(GNNGLS_PROF_TRAIN_GAT_BWD, st);
          GNNGLS_TRY(launch_attention_bwd(plan.bwd, ft, db, g, att, p.attn_l, p.attn_r, B, n, part, pms, st)); }
        { ProfScope ps(GNNGLS_PROF_TRAIN_ELEMENTWISE, st);
          GNNGLS_TRY(launch_attention_bwd_combine(plan.combine, part, pms, p.attn_l, p.attn_r, M, dft, dl, dr, st)); }
        { ProfScope ps(GNNGLS_PROF_TRAIN_COLSUM, st);
          if (plan.combine == gnngls::COMBINE_HEADS16) {
              nb = gnngls::colsum_blocks(M, 128);
              GNNGLS_TRY(gnngls::launch_colsum_heads16(ft, dl, dr, M, csp, nb, st));
          } else GNNGLS_TRY(gnngls::launch_colsum(gnngls::CS_HEADSCALE, ft, dl, dr, M, 128, 0, csp, &nb, st));
          GNNGLS_TRY(gnngls::launch_colsum_store(csp, nb, 128, 1, d.attn_l, d.attn_r, st)); }
        { ProfScope ps(GNNGLS_PROF_TRAIN_GEMM_TN, st);
          GNNGLS_TRY(gnngls::launch_gemm_tn(dft, h, M, 128, 128, tnp, d.fc_w, nullptr, st)); }
        { ProfScope ps(GNNGLS_PROF_TRAIN_GEMM_BWD, st);      // d h = d ft * Wfc + d h1 (skip, models.py:15)
          GNNGLS_TRY(gnngls::launch_gemm_wkn(gnngls::GEMM_EPI_ADD, dft, p.fc_w, da, M, 128, 128, db, st)); }
    }
    // embedding (models.py:66): h0 = x We^T + be
    { ProfScope ps(GNNGLS_PROF_TRAIN_COLSUM, st);
      for (int d = 0; d < in_dim; ++d) {
          GNNGLS_TRY(gnngls::launch_colsum(gnngls::CS_ROWSCALE, da, feat + d, nullptr, M, 128, in_dim, csp, &nb, st));
          GNNGLS_TRY(gnngls::launch_colsum_store(csp, nb, 128, in_dim, g_emb_w + d, d == 0 ? g_emb_b : nullptr, st));
      } }
    return GNNGLS_OK;
}

#undef GNNGLS_TRY

}  // extern "C"

// ---------------------------------------------------------------------------------------------
// per-kernel-class timing
// ---------------------------------------------------------------------------------------------
extern "C" {

int gnngls_debug_set_penalty16_limit(int limit) {
    if (limit < 1 || limit > 65535) return fail(GNNGLS_ERR_ARG, "penalty16 limit must be in 1..65535");
    g_pen16_limit = limit;
    return GNNGLS_OK;
}

int gnngls_profile_set_executed_evals(int64_t *device_buffer) {
    g_exec_evals.store((long long *)device_buffer, std::memory_order_relaxed);
    return GNNGLS_OK;
}

int gnngls_debug_set_gls_prune(int mode) {
    if (mode < -1 || mode > 1) return fail(GNNGLS_ERR_ARG, "gls prune mode must be -1 (default: on), 0 (full scans) or 1 (on)");
    g_prune_mode.store(mode, std::memory_order_relaxed);
    return GNNGLS_OK;
}

int gnngls_debug_set_gls_team(int mode) {
    if (mode < -1 || mode > 1) return fail(GNNGLS_ERR_ARG, "gls team mode must be -1 (policy), 0 (never) or 1 (wherever it exists)");
    g_team_mode.store(mode, std::memory_order_relaxed);
    return GNNGLS_OK;
}

int gnngls_debug_set_gls_threads(int threads) {
    // 1024 is not accepted: only the 128-VGPR instantiations are compiled for 16-wave workgroups (the default policy
    // picks them itself where a workgroup owns a CU); the 64- and 80-VGPR builds are bounded at 512 threads
    if (threads != 0 && threads != 64 && threads != 128 && threads != 256 && threads != 512)
        return fail(GNNGLS_ERR_ARG, "gls threads override must be 0 (default policy), 64, 128, 256 or 512");
    g_threads_override.store(threads, std::memory_order_relaxed);
    return GNNGLS_OK;
}

int gnngls_debug_set_stamp_buffer(void *device_buffer) {
    g_stamp_buffer = (long long *)device_buffer;
    return GNNGLS_OK;
}

int gnngls_profile_enable(int on) {
    std::lock_guard<std::mutex> lock(g_prof_mutex);
    for (auto &sp : g_spans) { (void)hipEventDestroy(sp.a); (void)hipEventDestroy(sp.b); }
    g_spans.clear();
    g_prof_on = on != 0;
    return GNNGLS_OK;
}

int gnngls_profile_collect(double *ms_by_kind, int64_t *launches_by_kind) {
    if (!ms_by_kind || !launches_by_kind) return fail(GNNGLS_ERR_ARG, "profile_collect: bad argument");
    for (int k = 0; k < GNNGLS_PROF_KINDS; ++k) { ms_by_kind[k] = 0.0; launches_by_kind[k] = 0; }
    std::vector<ProfSpan> spans;
    { std::lock_guard<std::mutex> lock(g_prof_mutex); spans.swap(g_spans); }
    for (auto &sp : spans) {
        hipError_t e = hipEventSynchronize(sp.b);
        if (e != hipSuccess) return hip_fail(e, "profile_collect");
        float ms = 0.f;
        e = hipEventElapsedTime(&ms, sp.a, sp.b);
        if (e != hipSuccess) return hip_fail(e, "profile_collect");
        ms_by_kind[sp.kind] += ms; launches_by_kind[sp.kind] += 1;
        (void)hipEventDestroy(sp.a); (void)hipEventDestroy(sp.b);
    }
    return GNNGLS_OK;
}

}  // extern "C"
