/*
 * include/gnngls_hip.h -- C ABI of libgnngls_hip.so (MI355X / gfx950).
 *
 * This is the drop-in boundary for the hot path of proroklab/gnngls (edge-regret GNN forward +
 * guided local search).  The reference has no FFI layer of its own: its boundary is the Python
 * call surface.  Each entry point below cites the reference function it
 * replaces (file:line into the reference tree); the gnngls_amd Python package binds them with ctypes and
 * re-exposes the reference's Python signatures (INTEGRATION.md shows the binding).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (hipMalloc / torch CUDA tensor .data_ptr()) unless the
 *     name ends in _host; buffers are caller-owned, contiguous, row-major; nothing is retained;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); calls only enqueue work;
 *   - B = number of independent TSP instances in the batch, n = nodes per instance;
 *     a tour is int32[n+1] with the depot (node 0) at both ends (algorithms.py:10,17);
 *     D is an n*n fp64 matrix indexed by node label (nx.attr_matrix, algorithms.py:140);
 *     N = n(n-1)/2 line-graph nodes (= TSP edges i<j in itertools.combinations order);
 *   - return value: 0 on success, negative on error; gnngls_last_error() gives the message.
 *     There is NO CPU fallback anywhere in this library.
 */
#ifndef GNNGLS_HIP_H
#define GNNGLS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GNNGLS_OK 0
#define GNNGLS_ERR_ARG (-1)
#define GNNGLS_ERR_HIP (-2)
#define GNNGLS_ERR_UNSUPPORTED (-3)

/* operator codes for gnngls_best_move */
#define GNNGLS_OP_TWO_OPT 0
#define GNNGLS_OP_RELOCATE 1

/* per-instance status words written by gnngls_gls_run */
#define GNNGLS_STATUS_OK 0
#define GNNGLS_STATUS_WATCHDOG 1      /* watchdog fired (search aborted, best-so-far returned) */
#define GNNGLS_STATUS_PENALTY_OVERFLOW 2   /* a 16-bit LDS penalty counter would pass 65535: rerun with penalty_bits=32 */
#define GNNGLS_STATUS_ASYMMETRIC 3    /* the instance's matrix is not bitwise symmetric and the run was on a store that keeps one
                                         triangle (every store but the global-memory one): NOT searched -- best = the start tour,
                                         0 iterations -- because the reference reads D[a,b] as indexed (operators.py:25-28,97-102)
                                         and the search would differ; rerun the instance with penalty_bits = -1 */
#define GNNGLS_STATUS_EDGE_LOST 4     /* gnngls_regret_labels: a fixed-edge search returned a tour without its edge (never expected:
                                         see there); that edge keeps its earlier label */
#define GNNGLS_STATUS_BAD_ORDER 5     /* gnngls_insertion, GNNGLS_INSERT_GIVEN_ORDER: the instance's row of `order` is not a
                                         permutation of the non-depot nodes; its tour row was left untouched */
#define GNNGLS_SAMPLE_BAD_WEIGHTS 6   /* gnngls_sample_nn_tours: a step of the walk met weights np.random.choice refuses (a NaN,
                                         negative or infinite probability, or a total that is not finite and positive); the
                                         walk's tour row is filled with -1 */

int gnngls_abi_version(void);
const char *gnngls_last_error(void);

/* Number of instances of size n that can be co-resident on the device for gnngls_gls_run
 * (one workgroup per instance, LDS-resident distance/penalty triangles); 0 if n needs the
 * global-memory fallback.  Host-side query, no device work. */
int gnngls_gls_resident_capacity(int n);

/* Host-side query: the storage configuration gnngls_gls_run would use for B instances of n nodes.
 *   *store     0 = global-memory store, 116 / 132 = distance + 16/32-bit penalty triangles in LDS,
 *              200 = compact store (distance triangle in LDS, penalties in global memory)
 *   *threads   workgroup size, *lds_bytes dynamic LDS per workgroup, *per_cu resident workgroups per CU (0: n/a) */
int gnngls_gls_describe_config(int n, int B, int penalty_bits, int *store, int *threads, int *lds_bytes, int *per_cu);

/* The same query for exactly the launch gnngls_gls_run(…, first_improvement, penalty_bits, …) makes (ABI v3).  The three
 * older queries -- gnngls_gls_describe_config, gnngls_gls_waves_per_simd, gnngls_gls_uses_team -- answer for a
 * best-improvement run; a first-improvement run can use another workgroup size (n = 25..33), register budget and form of
 * the perturbation phase.  *waves_per_simd, *team as documented there; *edge_form = 1 if the serial perturbation phase
 * (algorithms.py:150-185) runs in its edge form (tour edges in registers; symmetric stores, 32-bit counters, best
 * improvement), 0 for the scan-by-scan form.  Any output pointer may be NULL. */
int gnngls_gls_describe_run(int n, int B, int penalty_bits, int first_improvement, int *store, int *threads, int *lds_bytes,
                            int *per_cu, int *waves_per_simd, int *team, int *edge_form);

/* Vector registers per lane and scratch bytes per lane of the kernel instantiation that launch would run (trace != 0: with a
 * per-move trace buffer) -- hipFuncGetAttributes on the selected function, so it needs the device.  Every BASELINE.json shape
 * runs on an instantiation without scratch; tests/test_perf_floor_gpu.py asserts it so that a code-generation regression in
 * this ~70-instantiation kernel shows in the driver's GPU tests. */
int gnngls_gls_kernel_resources(int n, int B, int penalty_bits, int first_improvement, int trace, int *vgprs, int *scratch_bytes);

/* ---- K3u: move-evaluation tables (parity/unit kernels) ---------------------------------------
 * out[b][i][j] (shape [B, n+1, n+1]) = two_opt_cost(tour_b, D_b, i, j)   operators.py:14-29
 *                                    = relocate_cost(tour_b, D_b, i, j)  operators.py:83-103
 * for 1 <= i,j <= n-1; NaN elsewhere.  D may be asymmetric (index order follows the reference). */
int gnngls_two_opt_delta_all(const int32_t *tour, const double *D, int B, int n, double *out, void *stream);
int gnngls_relocate_delta_all(const int32_t *tour, const double *D, int B, int n, double *out, void *stream);

/* ---- one scan of a move operator --------------------------------------------------------------
 * op = GNNGLS_OP_TWO_OPT : two_opt_a2a (operators.py:32-50) / two_opt_o2a (operators.py:53-73)
 * op = GNNGLS_OP_RELOCATE: relocate_a2a (operators.py:129-147) / relocate_o2a (operators.py:106-126)
 * pos_i == NULL -> all-to-all scan; else one-to-all from position pos_i[b] (must be in 1..n-1,
 * the reference asserts this at operators.py:54,107; violating it returns GNNGLS_ERR_ARG only if
 * checked on the host side by the caller -- the kernel clamps nothing).
 * Acceptance rule operators.py:42,65,118,139: delta < best and not np.isclose(0, delta).
 * Outputs: delta_out[b] (0.0 if no move), move_out[b] = {i, j} ({0,0} if none),
 *          new_tour[b] = tour after the move (copy of the input if none). */
int gnngls_best_move(const int32_t *tour, const double *D, int B, int n, int op, const int32_t *pos_i,
                     int first_improvement, double *delta_out, int32_t *move_out, int32_t *new_tour,
                     void *stream);

/* ---- tour_cost (gnngls/__init__.py:17-21): sequential left-to-right fp64 sum ------------------ */
int gnngls_tour_cost(const int32_t *tour, const double *D, int B, int n, double *cost_out, void *stream);

/* ---- nearest_neighbor (algorithms.py:9-18) on a dense weight matrix W[B,n,n]; ties -> lowest id */
int gnngls_nearest_neighbor(const double *W, int B, int n, int depot, int32_t *tour_out, void *stream);

/* ---- insertion (algorithms.py:82-108): the closed tour grows from [depot, depot] by one node per step ---------------------
 * mode GNNGLS_INSERT_NEAREST / _FARTHEST: the next node is the outside node j of the pair (tour member i, j) with the smallest /
 *      largest W[i,j] (algorithms.py:93-103: `for i in tour: for j in nodes` with a strict compare, so ties go to the smallest
 *      tour position of i, then to the smallest j);
 * mode GNNGLS_INSERT_GIVEN_ORDER: the next node is order[b][step] -- mode 'random' of the reference (algorithms.py:90-91),
 *      whose np.random.choice draws do not depend on the tour; the caller makes them on the host (gnngls_amd.ops.random_order).
 * Each node goes where cheapest_insertion (below) puts it.
 *   W         [B,n,n] fp64, finite; the reference reads an undirected graph, so only symmetric matrices are pinned to it: the
 *             kernel reads W[t[p], t[p+1]] in tour direction and W[i,j] with i the tour member.  With NaN weights the tours
 *             are unspecified (every index stays in range).
 *   order     [B,n-1] int32 and status [B]: required for GNNGLS_INSERT_GIVEN_ORDER only (status, when given, is written 0 in the
 *             other modes).  The kernel checks every row of `order` to be a permutation of the non-depot nodes BEFORE it uses an
 *             entry as an index: a bad row gets status GNNGLS_STATUS_BAD_ORDER, its row of tour_out is left untouched and
 *             nothing is read or written out of range.
 *   tour_out  [B,n+1]; n = 1 gives [d, d], n = 2 gives [d, x, d].
 * 1 <= n <= GNNGLS_INSERTION_MAX_N (one workgroup per instance, 48 B of LDS per node); a larger n returns
 * GNNGLS_ERR_UNSUPPORTED.  Bad arguments are rejected on the host before any device work; B == 0 returns GNNGLS_OK. */
#define GNNGLS_INSERT_NEAREST 0
#define GNNGLS_INSERT_FARTHEST 1
#define GNNGLS_INSERT_GIVEN_ORDER 2
#define GNNGLS_INSERTION_MAX_N 2048
int gnngls_insertion(const double *W, int B, int n, int depot, int mode, const int32_t *order, int32_t *tour_out,
                     int32_t *status, void *stream);

/* ---- cheapest_insertion (algorithms.py:67-79): one step on a caller's sub-tour ------------------------------------------------
 * For every position j = 1 .. len-1 the candidate is sub_tour with `node` inserted at j; its cost is tour_cost
 * (gnngls/__init__.py:17-21): the left-to-right fp64 sum of ALL its edge weights, not a difference against the old tour.  The
 * first j whose cost is strictly smallest wins (algorithms.py:76).
 *   sub_tour  [B,len] int32 (any node list, usually closed: [d, ..., d]), 2 <= len <= n (the reference returns None for
 *             len < 2: gnngls_amd.algorithms does that on the host); node [B]; W [B,n,n] as above, 1 <= n <= GNNGLS_INSERTION_MAX_N
 *   tour_out  [B,len+1], cost_out [B] the winning candidate's tour_cost.  An instance with an index out of 0..n-1 in its
 *             sub-tour or node gets cost NaN and its tour row untouched; nothing is read out of range. */
int gnngls_cheapest_insertion(const int32_t *sub_tour, int len, const int32_t *node, const double *W, int B, int n,
                              int32_t *tour_out, double *cost_out, void *stream);

/* ---- Held-Karp 1-tree lower bound of the optimal tour length (oracle/one_tree.c: one_tree_lower_bound, min_one_tree) --------
 * The reference divides a tour's length by Concorde's optimum stored in its instance files (scripts/test.py:62,104,
 * gnngls/__init__.py:55-60).  This entry gives the certified side this project can compute itself: for node potentials pi,
 *      w(pi) = min over 1-trees of (c[i][j] + pi[i] + pi[j])  -  2 sum(pi)   <=   optimum,
 * and the subgradient ascent of oracle/one_tree.c (Polyak steps towards ub, the step factor halved after `period` 1-trees
 * without a better value: period = 25 below n = 50, else n / 2) returns max_k w(pi_k).  The kernel repeats that file's fp64
 * operations in its order: `bound` has the bits of one_tree_lower_bound(D_b, n, ub_b, max_iters).  On uniform instances the bound
 * lies typically 0.7-1 % below the optimum; where the ascent lands on a tour (most instances up to n ~ 20) it IS the optimum.
 *   D         [B,n,n] fp64, finite (non-finite entries: unspecified values, every index stays in range), bitwise symmetric: an
 *             instance whose matrix is not gets status GNNGLS_STATUS_ASYMMETRIC, bound NaN and its other outputs untouched
 *             (one pass over the matrix before the ascent; w(pi) is a bound for symmetric costs only);
 *   ub        [B] the length of any tour of the instance (it steers the step size only; ub <= w falls back to 1e-3 ub, or 1e-3);
 *   max_iters >= 0, the largest number of 1-trees built (the oracle's default is 2000);
 *   bound     [B] max_k w(pi_k) (-DBL_MAX with max_iters = 0);
 *   pi        [B,n] or NULL: the potentials that attain it (the oracle's best_pi, which it does not return) -- the root of a
 *             branch and bound;
 *   iters     [B] 1-trees built;  exit_kind [B] GNNGLS_BOUND_EXIT_*;  status [B] 0 or GNNGLS_STATUS_ASYMMETRIC.
 * One workgroup per instance and one launch for the whole batch; every loop is bounded by max_iters x n.
 * 3 <= n <= GNNGLS_ONE_TREE_MAX_N (a larger n returns GNNGLS_ERR_UNSUPPORTED; the oracle's n < 3 branch is not reproduced).  Bad
 * arguments are rejected on the host before any device work; B == 0 returns GNNGLS_OK. */
#define GNNGLS_ONE_TREE_MAX_N 1024
#define GNNGLS_BOUND_EXIT_ITERS 0     /* max_iters 1-trees were built */
#define GNNGLS_BOUND_EXIT_STEP 1      /* the step factor fell to 1e-5 */
#define GNNGLS_BOUND_EXIT_TOUR 2      /* the minimum 1-tree is a tour: the bound is the optimum */
int gnngls_one_tree_bound(const double *D, const double *ub, int B, int n, int max_iters, double *bound, double *pi, int32_t *iters,
                          int32_t *exit_kind, int32_t *status, void *stream);

/* ---- alpha-nearness (Helsgaun): a model-free, regret-like search guide from the 1-tree -----------------------------------------
 * alpha(e) = (cost of the minimum 1-tree forced through e) - (cost of the minimum 1-tree) under node potentials pi, the
 * classical relaxation of the regret the model predicts ((best tour through e - optimum) / optimum).  With the pi of
 * gnngls_one_tree_bound it is the guide a search takes in place of a model's prediction.  Definition (the contract):
 *   D [B,n,n] fp64 bitwise symmetric, pi [B,n] fp64 or NULL (all zeros), 3 <= n <= GNNGLS_ALPHA_MAX_N; node 0 is the special
 *   node, as in gnngls_one_tree_bound and oracle/one_tree.c; every operation below is one fp64 operation rounded once.
 *   Canonical weight: w(i,j) = ((D[i][j] + pi[min(i,j)]) + pi[max(i,j)]) + 0.0 -- the potential of the smaller node first, so
 *   that w(i,j) == w(j,i) bit for bit (the bound's (row + pi[u]) + pi[v] depends on which endpoint entered the tree first;
 *   alpha must not); the last term only reads a weight of -0.0 as +0.0.
 *   Pairs 1 <= i < j: beta(i,j) = the largest w on the path between i and j in a minimum spanning tree of nodes 1..n-1 under w
 *   -- the minimax-path value, the same for every minimum spanning tree -- and alpha(i,j) = w(i,j) - beta(i,j).
 *   Pairs with node 0: m2 = the second smallest of w(0,j), j = 1..n-1, counted with multiplicity;
 *   alpha(0,j) = w(0,j) - m2 if that is > 0, else +0.0.
 *   alpha [B,n,n] fp64 is bitwise symmetric with a +0.0 diagonal.
 * Every beta is one of the w, selected by comparisons and never computed: alpha is bit-determined by (D, pi) and does not depend
 * on the tie-breaks inside Prim; it is >= 0, and on an instance without ties exactly n unordered pairs -- the edges of the
 * minimum 1-tree -- have alpha = +0.0.  gnngls_amd.host.alpha_nearness restates the definition in NumPy.
 *   status [B]: 0, or GNNGLS_STATUS_ASYMMETRIC for an instance whose matrix is not bitwise symmetric (one pass in front of Prim);
 *   that instance's alpha is filled with NaN.  Non-finite costs or potentials: unspecified values, every index stays in range.
 * One workgroup per instance, one launch for the batch, O(n^2) work per instance (ONE spanning tree, where the ascent of
 * gnngls_one_tree_bound builds up to max_iters).  Bad arguments -- a NULL D, alpha or status, B < 1, n < 3 (GNNGLS_ERR_ARG),
 * n > GNNGLS_ALPHA_MAX_N (GNNGLS_ERR_UNSUPPORTED) -- are rejected on the host before any device work. */
#define GNNGLS_ALPHA_MAX_N 1024
int gnngls_alpha_nearness(const double *D, const double *pi, int B, int n, double *alpha, int32_t *status, void *stream);

/* ---- Or-opt: a chain of one to three consecutive tour nodes moves between two other tour neighbours, forward or reversed ------
 * The reference's only node-moving operator is relocate (operators.py:76-147), which moves one node; Or-opt is its
 * generalisation to short chains, the operator KGLS runs beside 2-opt.  Definition (the contract):
 *   tour t[0..n], t[0] = t[n] = the depot; positions 1..n-1 move, the depot never does.  A candidate is (i, L, rev, j):
 *   the chain S = t[i .. i+L-1] with 1 <= i, i+L-1 <= n-1, 1 <= L <= max_seg <= GNNGLS_OR_OPT_MAX_SEG; t' = t with S removed
 *   (length n+1-L; t'[q] = t[q] for q < i, else t[q+L]); j in 1..n-L is the index at which S lands in t' -- the list.insert
 *   index of the reference's relocate; rev in {0, 1}, rev = 1 only for L >= 2 and only when `reverse` is set.
 *   a = t[i-1], s1 = t[i], sL = t[i+L-1], c = t[i+L], d = t'[j-1], e = t'[j].
 *   Skipped: j == i in both orientations (the identity, or an in-place reversal, which 2-opt owns), and rev == 0 with j == i-1
 *   (the reference's `i - j == 1` rule, operators.py:135).
 *   delta, fp64, evaluated left to right exactly as written, every operation rounded once:
 *     rev = 0:  -D[a,s1] - D[sL,c] + D[a,c] - D[d,e] + D[d,s1] + D[sL,e]
 *     rev = 1:  -D[a,s1] - D[sL,c] + D[a,c] - D[d,e] + D[d,sL] + D[s1,e]
 *   For L = 1 this is relocate_cost (operators.py:97-102) operand by operand.
 *   Acceptance is the reference's: delta < best_delta and not np.isclose(0, delta) (operators.py:139).  Candidates are enumerated
 *   in ascending lexicographic order of (i, L, rev, j); the chosen move is the first candidate with the smallest qualifying
 *   delta.  The tour after the move is t'[:j] + S (or S reversed) + t'[j:].
 *   D [B,n,n] must be bitwise symmetric (the kernels read D[d,s1] as D[s1][d]; one pass in front of the first scan checks it);
 *   tour entries are node ids in 0..n-1 (the kernels clamp nothing).  gnngls_amd.host restates all of it in NumPy.
 * gnngls_or_opt_best_move: one scan.  delta [B] = the chosen move's delta, 0.0 when no candidate qualifies, NaN for an instance
 *   whose matrix is not bitwise symmetric; move [B,4] = i, L, rev, j (-1s when none); new_tour [B,n+1] = the tour after the move
 *   (the input when none).
 * gnngls_or_opt_descent: local_search (algorithms.py:111-132) with relocate_a2a replaced by the scan above -- two_opt_a2a
 *   (operators.py:32-50) and the Or-opt scan alternate, best improvement; after each move cost += delta; the loop ends when a
 *   full pass moves nothing, or after max_moves applied moves (checked after every move).  With max_seg = 1 and reverse = 0 it
 *   is the reference's local_search bit for bit.
 *   tour [B,n+1], cost [B] the start tours and their lengths; tour_out, cost_out the result; moves [B] applied moves;
 *   trace_cost [B,trace_cap] or NULL: the cost after each of the first trace_cap moves (later entries untouched).
 *   status [B]: GNNGLS_STATUS_OK (a local optimum of both scans), GNNGLS_STATUS_MOVE_CAP (the cap ended the run, even where
 *   the tour happens to be a local optimum), or GNNGLS_STATUS_ASYMMETRIC (not searched: the outputs are the inputs, 0 moves).
 *   A NaN fails every comparison of the acceptance rule, so an instance with NaN costs stops at once.
 * One workgroup per instance, one launch for the batch; the loop is bounded by max_moves: no watchdog, no wall clock.
 * 3 <= n <= GNNGLS_OR_OPT_MAX_N (a larger n returns GNNGLS_ERR_UNSUPPORTED).  Bad arguments -- a NULL pointer other than
 * trace_cost, B < 1, n < 3, max_seg outside 1..GNNGLS_OR_OPT_MAX_SEG, max_moves < 1, trace_cap < 0 (GNNGLS_ERR_ARG) -- are
 * rejected on the host before any device work. */
#define GNNGLS_OR_OPT_MAX_N 1024
#define GNNGLS_OR_OPT_MAX_SEG 3
#define GNNGLS_STATUS_MOVE_CAP 6      /* gnngls_or_opt_descent: max_moves moves were applied and the run ended there */
int gnngls_or_opt_best_move(const int32_t *tour, const double *D, int B, int n, int max_seg, int reverse, double *delta,
                            int32_t *move, int32_t *new_tour, void *stream);
int gnngls_or_opt_descent(const int32_t *tour, const double *cost, const double *D, int B, int n, int max_seg, int reverse,
                          int max_moves, int32_t *tour_out, double *cost_out, int32_t *moves, int32_t *status, double *trace_cost,
                          int trace_cap, void *stream);

/* ---- iterated local search: double-bridge kicks around the descent of gnngls_or_opt_descent, one launch -----------------------
 * The second metaheuristic beside guided local search: kick the local optimum, descend again, keep the better tour.  The
 * reference has no counterpart.  Definition (the contract; gnngls_amd.host.ils restates it in NumPy, bit for bit):
 *   tour t[0..n], t[0] = t[n] = the depot, m = n - 1, D [B,n,n] fp64 bitwise symmetric.
 *   Cut points from three uniforms u0, u1, u2 in [0,1); each product is one fp64 multiply, truncated toward zero, then clamped
 *   into its range (the device also clamps below at 0; a u outside [0,1) or a NaN still gives a closed permutation -- which one
 *   is unspecified, as for the sampled walks below):
 *     p1 = 1 + min(int(u0 * (m - 2)), m - 3)                      1 .. m-2
 *     p2 = p1 + 1 + min(int(u1 * (m - 1 - p1)), m - 2 - p1)       p1+1 .. m-1
 *     p3 = p2 + 1 + min(int(u2 * (m - p2)), m - 1 - p2)           p2+1 .. m
 *   Kick: the orientation-preserving double bridge.  A = t[0:p1], B = t[p1:p2], C = t[p2:p3], Dseg = t[p3:n]; the new tour is
 *   A + Dseg + C + B + [t[n]] -- A D C B: all four junctions are new (A C B D would only be a segment swap); the depot never
 *   moves.  With ae = t[p1-1], bs = t[p1], be = t[p2-1], cs = t[p2], ce = t[p3-1], ds = t[p3], de = t[n-1], z = t[n] its delta is,
 *   fp64, left to right as written, every operation rounded once:
 *     D[ae,ds] + D[de,cs] + D[ce,bs] + D[be,z] - D[ae,bs] - D[be,cs] - D[ce,ds] - D[de,z]
 *   Run:
 *     1. cur, cur_cost = the descent of gnngls_or_opt_descent (max_seg, reverse) from (tour, cost).
 *     2. for k = 0 .. kicks-1: cand = kick(cur), cand_cost = cur_cost + delta; cand, cand_cost = the same descent from there;
 *        trace_cost[k] = cand_cost; d = cand_cost - cur_cost; accept iff d < 0 and not np.isclose(0, d) (the reference's
 *        acceptance rule, operators.py:42, applied to the kick: the accumulated costs of one tour reached by two paths differ in
 *        their last bits); when accepted cur, cur_cost = cand, cand_cost and accepted += 1.
 *     3. max_moves caps the applied descent moves of the whole run, checked after every move: the descent in progress ends
 *        there, step 2's bookkeeping is applied to what it holds, and the run ends with GNNGLS_STATUS_MOVE_CAP.  The loop is
 *        bounded by kicks and max_moves only: no wall clock, no watchdog, no spin-wait.
 *   Uniforms: the caller's u [B,kicks,3] fp64, or with u == NULL Philox4x32-10 with key (seed & 0xffffffff, seed >> 32) and
 *   counter (b, kick0 + k, s, 1), s = 0, 1, 2; u = ((o0 << 32 | o1) >> 11) * 2^-53 -- the generator and formula of
 *   gnngls_sample_nn_tours; counter word 3 = 1 keeps the stream apart from the walks' (b, r, step, 0).
 *   kick0 >= 0 offsets the kick counter: a run of K1 kicks followed by a run of K2 kicks with kick0 = K1 from the first run's
 *   outputs IS a run of K1 + K2 kicks (the second run's first descent finds a local optimum and applies nothing) -- a host loop
 *   runs the search for a time budget in such rounds.  kicks = 0 is exactly gnngls_or_opt_descent.
 *   Outputs per instance: tour_out [B,n+1]; cost_out [B] the accumulated cost; moves [B] all applied descent moves, the first
 *   descent's included; accepted [B] accepted kicks; status [B] GNNGLS_STATUS_OK, GNNGLS_STATUS_MOVE_CAP or
 *   GNNGLS_STATUS_ASYMMETRIC (not searched: the outputs are the inputs); trace_cost [B,kicks] or NULL: entries of kicks that
 *   never ran stay as given.
 * One workgroup per instance, one launch for the batch, the tours resident in LDS (the accepted tour in a buffer of its own:
 * a rejected kick costs no copy).  4 <= n <= GNNGLS_OR_OPT_MAX_N (a larger n returns GNNGLS_ERR_UNSUPPORTED).  Bad arguments --
 * n < 4, B < 1, kicks < 0, kick0 < 0, kick0 + kicks > INT32_MAX, max_seg outside 1..GNNGLS_OR_OPT_MAX_SEG, max_moves < 1, a NULL
 * pointer other than u / trace_cost (GNNGLS_ERR_ARG) -- are rejected on the host before any device work. */
int gnngls_ils_run(const int32_t *tour, const double *cost, const double *D, int B, int n, int kicks, int kick0, int max_seg,
                   int reverse, int max_moves, uint64_t seed, const double *u, int32_t *tour_out, double *cost_out, int32_t *moves,
                   int32_t *accepted, int32_t *status, double *trace_cost, void *stream);

/* ---- guided local search over 2-opt and Or-opt, one launch, n <= GNNGLS_OR_OPT_MAX_N ------------------------------------------
 * The reference's guided_local_search (algorithms.py:135-195) with relocate_a2a and relocate_o2a replaced by the Or-opt scans --
 * the KGLS operator set the comment at algorithms.py:147 points to -- built on the descent of gnngls_or_opt_descent, for sizes
 * the LDS-resident stores of gnngls_gls_run do not reach.  Definition (the contract; gnngls_amd.host.two_opt_o2a, or_opt_o2a and
 * guided_or_opt restate it in NumPy, bit for bit):
 *   One-to-all scans at tour position i, 1 <= i <= n-1, on a matrix M:
 *     two_opt_o2a (operators.py:53-73): j = 1..n-1 with abs(i-j) >= 2; with lo = min(i,j), hi = max(i,j), a = t[lo], b = t[lo-1],
 *       c = t[hi], d = t[hi-1]:  delta = M[a,c] + M[b,d] - M[a,b] - M[c,d], left to right; the first j of the smallest delta with
 *       delta < best_delta and not np.isclose(0, delta); the move reverses t[lo .. hi-1].
 *     or_opt_o2a: the Or-opt candidates (s, L, rev, j) above whose chain t[s .. s+L-1] contains position i -- 1 <= s <= i <=
 *       s+L-1 <= n-1, 1 <= L <= max_seg -- in ascending (s, L, rev, j), the same delta and rule.  Only j == s is skipped, in both
 *       orientations: the rev == 0, j == s-1 skip of the all-to-all scan does NOT apply (relocate_o2a, operators.py:106-126,
 *       evaluates it, and its twin move is not in this set).  With max_seg = 1, reverse = 0 it is relocate_o2a operand by operand.
 *   gnngls_or_opt_o2a: one or_opt_o2a scan on D at pos[b] for every instance; the outputs are those of gnngls_or_opt_best_move
 *     (move = s, L, rev, j).  A position outside 1..n-1 has no candidates (delta 0.0, move -1s).
 *   Run (gnngls_guided_or_opt_run), per instance, with k = k[b], P = penalty[b] (int32 [n,n], symmetric, IN/OUT):
 *     1. cur, cur_cost = the descent of gnngls_or_opt_descent (max_seg, reverse) from (tour, cost); best = cur.
 *     2. for it = 0 .. outer_iters-1: guide = guides[(iter0 + it) % G][b]; moves_it = 0; while moves_it < perturbation_moves:
 *          the penalised edge (a, b) = (t[p], t[p+1]) of the first p with the greatest guide[a,b] / (1 + P[a,b]) (fp64; lines
 *          153-159: `util > max_util or max_util_e is None`; NaN utilities: which edge is unspecified);
 *          P[a,b] += 1, P[b,a] += 1;  Dg = D + k * P, elementwise, the product rounded, then the sum (never a fused multiply-add);
 *          for each of a, b, in this order, that is not the depot t[0]: i = the node's position in cur, taken ONCE (line 169);
 *          two_opt_o2a(cur, Dg, i), then or_opt_o2a(cur, Dg, i) on the tour the first one left; a found move replaces cur,
 *          cur_cost = the tour's cost under D summed left to right from 0 (line 176), moves_it += 1, trace_cost gets cur_cost.
 *        then cur, cur_cost = the descent from (cur, cur_cost) on D, and best = cur iff cur_cost < best_cost (plain <).
 *     3. max_moves counts the applied moves of every kind and is checked after each; max_steps counts penalisations and is
 *        checked before each.  A cap ends the run where it stands, the `cur_cost < best_cost` bookkeeping is applied to what the
 *        run holds, and the status is GNNGLS_STATUS_MOVE_CAP / GNNGLS_STATUS_STEP_CAP.  The run is bounded by outer_iters and
 *        the two caps only: no wall clock, no watchdog, no spin-wait, nothing shared between workgroups.
 *   With max_seg = 1 and reverse = 0, k = 0.1 * cost / n and zeroed penalties the best tour, its cost, the trace and the
 *   penalties are those of guided_local_search run for outer_iters iterations, bit for bit (gnngls_gls_run, max_outer_iters).
 *   iter0 >= 0 offsets the guide index: a run of K1 iterations followed by a run of K2 with iter0 = K1 from the first run's
 *   CURRENT tour, cost and penalties under the same k IS a run of K1 + K2 iterations (the second run's first descent applies
 *   nothing); the caller keeps the better of the two bests under <, ties to the earlier.
 *   Outputs per instance: tour_out, cost_out the current tour and its cost; best_tour, best_cost; moves [B] all applied moves;
 *   steps [B] penalisations; status [B] GNNGLS_STATUS_OK, GNNGLS_STATUS_MOVE_CAP, GNNGLS_STATUS_STEP_CAP or
 *   GNNGLS_STATUS_ASYMMETRIC (D is not bitwise symmetric: not searched, the outputs are the inputs, the penalties untouched);
 *   trace_cost [B,trace_cap] or NULL: the cost after each of the first trace_cap applied moves (later entries untouched);
 *   trace_len [B] or NULL: min(moves, trace_cap).
 * One workgroup per instance, one launch for the batch; the tours live in LDS, D, the guides and the penalties in global memory.
 * 4 <= n <= GNNGLS_OR_OPT_MAX_N (a larger n returns GNNGLS_ERR_UNSUPPORTED).  Bad arguments -- n < 4 (gnngls_or_opt_o2a: n < 3),
 * B < 1, outer_iters < 0, iter0 < 0, iter0 + outer_iters > INT32_MAX, outer_iters > 0 with G < 1 or guides NULL,
 * perturbation_moves < 0, max_seg outside 1..GNNGLS_OR_OPT_MAX_SEG, max_moves < 1, max_steps < 1, trace_cap < 0, a NULL pointer
 * other than guides / trace_cost / trace_len (GNNGLS_ERR_ARG) -- are rejected on the host before any device work. */
#define GNNGLS_STATUS_STEP_CAP 7      /* gnngls_guided_or_opt_run: max_steps penalisations were made and the run ended there */
int gnngls_or_opt_o2a(const int32_t *tour, const double *D, const int32_t *pos, int B, int n, int max_seg, int reverse, double *delta,
                      int32_t *move, int32_t *new_tour, void *stream);
int gnngls_guided_or_opt_run(const int32_t *tour, const double *cost, const double *D, const double *guides, int G, const double *k,
                             int32_t *penalty, int B, int n, int outer_iters, int iter0, int perturbation_moves, int max_seg,
                             int reverse, int max_moves, int max_steps, int32_t *tour_out, double *cost_out, int32_t *best_tour,
                             double *best_cost, int32_t *moves, int32_t *steps, int32_t *status, double *trace_cost, int trace_cap,
                             int32_t *trace_len, void *stream);

/* ---- 3-opt: three tour edges leave and the pieces between them are reconnected in every way that is no 2-opt move -------------
 * The upper end of the classical family beside 2-opt, relocate and Or-opt: every Or-opt candidate above, with any max_seg and
 * reversed or not, is a 3-opt move of the same tour.  The reference has no counterpart.  Definition (the contract;
 * gnngls_amd.host restates it in NumPy, bit for bit):
 *   tour t[0..n], t[0] = t[n] = the depot.  The tour edge at position p is (t[p], t[p+1]), p = 0..n-1.  A candidate is
 *   (p1, p2, p3, kind) with 0 <= p1 < p2 < p3 <= n-1 and kind in 0..3.  Removing the three edges leaves the head H = t[0..p1],
 *   B = t[p1+1..p2], C = t[p2+1..p3] and the tail T = t[p3+1..n]; head and tail stay, so the depot never moves.
 *   a1 = t[p1], b1 = t[p1+1], b2 = t[p2], c1 = t[p2+1], c2 = t[p3], a2 = t[p3+1].
 *     kind 0:  H + B reversed + C reversed + T    added edges, in this order: D[a1,b2], D[b1,c2], D[c1,a2]
 *     kind 1:  H + C + B + T                                                  D[a1,c1], D[c2,b1], D[b2,a2]
 *     kind 2:  H + C reversed + B + T                                         D[a1,c2], D[c1,b1], D[b2,a2]
 *     kind 3:  H + C + B reversed + T                                         D[a1,c1], D[c2,b2], D[b1,a2]
 *   delta, fp64, evaluated left to right exactly as written, every operation rounded once, with x, y, z the kind's added edges:
 *     delta = ((((x + y) + z) - D[a1,b1]) - D[b2,c1]) - D[c2,a2]
 *   Degenerate candidates (|B| = 1 or |C| = 1: a kind reproduces a 2-opt tour or another kind's tour) stay in the enumeration:
 *   they are valid tours and the tie rule decides between them.
 *   Acceptance is the reference's: delta < best_delta and not np.isclose(0, delta) (operators.py:42).  Candidates are enumerated
 *   in ascending lexicographic order of (p1, p2, p3, kind); the chosen move is the first candidate with the smallest qualifying
 *   delta.  Nothing is pruned: a scan evaluates all C(n,3) x 4 candidates.
 *   D [B,n,n] must be bitwise symmetric (the kernels read D[c2,b1] as D[b1][c2]; one pass in front of the first scan checks it);
 *   tour entries are node ids in 0..n-1 (the kernels clamp nothing).
 * gnngls_three_opt_best_move: one scan.  delta [B] = the chosen move's delta, 0.0 when no candidate qualifies, NaN for an
 *   instance whose matrix is not bitwise symmetric; move [B,4] = p1, p2, p3, kind (-1s when none); new_tour [B,n+1] = the tour
 *   after the move (the input when none).
 * gnngls_three_opt_descent: local_search (algorithms.py:111-132) with relocate_a2a replaced by the scan above -- two_opt_a2a
 *   (operators.py:32-50) and the 3-opt scan alternate, best improvement; after each move cost += delta; the loop ends when a
 *   full pass moves nothing, or after max_moves applied moves (checked after every move).
 *   tour [B,n+1], cost [B] the start tours and their lengths; tour_out, cost_out the result; moves [B] applied moves;
 *   trace_cost [B,trace_cap] (NULL only with trace_cap 0): the cost after each of the first trace_cap moves (later entries
 *   untouched).
 *   status [B]: GNNGLS_STATUS_OK (a local optimum of both scans), GNNGLS_STATUS_MOVE_CAP (the cap ended the run, even where
 *   the tour happens to be a local optimum), or GNNGLS_STATUS_ASYMMETRIC (not searched: the outputs are the inputs, 0 moves).
 *   A NaN fails every comparison of the acceptance rule, so an instance with NaN costs stops at once.
 * One workgroup per instance, one launch for the batch; the loop is bounded by max_moves: no watchdog, no wall clock.
 * 3 <= n <= GNNGLS_THREE_OPT_MAX_N (a position takes eight bits of the selection key, and one workgroup's O(n^3) scan is of no
 * use beyond it; a larger n returns GNNGLS_ERR_UNSUPPORTED; n = 3 has one triple and never moves).  Bad arguments -- a NULL
 * pointer (trace_cost: with trace_cap > 0), B < 1, n < 3, max_moves < 1, trace_cap < 0 (GNNGLS_ERR_ARG) -- are rejected on the
 * host before any device work.  gnngls_three_opt_lds_max_n: the largest n whose distance triangle this build stages in LDS
 * (larger instances read D from global memory; the results are the same bit for bit). */
#define GNNGLS_THREE_OPT_MAX_N 256
int gnngls_three_opt_best_move(const int32_t *tour, const double *D, int B, int n, double *delta, int32_t *move, int32_t *new_tour,
                               void *stream);
int gnngls_three_opt_descent(const int32_t *tour, const double *cost, const double *D, int B, int n, int max_moves, int32_t *tour_out,
                             double *cost_out, int32_t *moves, int32_t *status, double *trace_cost, int trace_cap, void *stream);
int gnngls_three_opt_lds_max_n(void);

/* ---- sampled nearest-neighbour walks (algorithms.py:21-50: probabilistic_nearest_neighbour) ----------------------------------
 * R independent walks per instance, one wavefront each, one launch for the B * R walks.  Walk (b, r):
 *   tour = [depot]; at every step i = tour[-1] and the candidates are the unvisited nodes j in ascending id, g_j = W[b,i,j];
 *   p = g; if any g_j is +-inf then p_j = 1.0 where g_j is infinite and 0.0 elsewhere (:34-36); if the sum of p is 0 then every
 *   p_j = 1.0 (:39-40); if `invert` then p_j = 1 / p_j (:43-44);
 *   where the reference's np.random.choice would raise -- some p_j is NaN, negative or infinite, or the total is not finite and
 *   positive (a zero weight under `invert` is such a case) -- the walk stops: status[b,r] = GNNGLS_SAMPLE_BAD_WEIGHTS and its row
 *   of `tours` is filled with -1;
 *   draw: x = u * total; the first candidate with p_j > 0 whose running sum exceeds x, or, if rounding leaves none, the last
 *   candidate with p_j > 0 (a candidate of weight zero could be the first to exceed x only through rounding: it is never picked).
 * Summation order (it decides ties at a boundary, so it is part of the definition).  Node j sits on lane j % 64, slot j / 64; a
 * node that is no candidate contributes +0.0.  For slot s = 0, 1, .. in order: c_s = the inclusive doubling scan of the slot over
 * its 64 lanes (for d = 1, 2, 4, 8, 16, 32 in order every lane l >= d adds the value lane l - d held before the round);
 * running sum of node j = base_s + c_s[j % 64] with base_0 = +0.0 and base_{s+1} = base_s + c_s[63]; total = the last base.  The
 * sum of the all-zero rule is this total on the p before inversion.  Every step is one fp64 operation rounded once.
 * Uniforms: u[b,r,s] in [0,1) for step s = 0 .. n-2 (the last step draws too, as the reference does) -- the caller's array, or with
 * u == NULL the 53-bit uniform ((o0 << 32 | o1) >> 11) * 2^-53 of Philox4x32-10 with key (seed & 0xffffffff, seed >> 32) and
 * counter (b, r, s, 0), (o0, o1) its first two output words.  A walk therefore depends on its instance's matrix and its own
 * uniforms only, never on the launch shape or on its neighbours.  The draws are NOT NumPy's: given `u` the walk is pinned bit for
 * bit (tests/test_sampling_cpu.py restates it in NumPy), against the reference it is pinned in law.
 *   W [B,n,n] fp64 (read as indexed: W[b,i,j] with i the current node); tours [B,R,n+1] int32 closed tours from `depot`;
 *   status [B,R] int32 0 or GNNGLS_SAMPLE_BAD_WEIGHTS.  A u outside [0,1) still yields a closed permutation (which: unspecified).
 * 3 <= n <= GNNGLS_SAMPLE_MAX_N (visited bits and candidate weights stay in registers, 16 nodes per lane at most; a larger n
 * returns GNNGLS_ERR_UNSUPPORTED), R >= 1, B * R < 2^31.  Bad arguments are rejected on the host before any device work; B == 0
 * returns GNNGLS_OK. */
#define GNNGLS_SAMPLE_MAX_N 1024
int gnngls_sample_nn_tours(const double *W, int B, int n, int R, int depot, int invert, uint64_t seed, const double *u,
                           int32_t *tours, int32_t *status, void *stream);

/* ---- ant colony optimisation: a MAX-MIN ant system (Stuetzle & Hoos) over any edge heuristic ----------------------------------
 * The second established use of an edge score beside the utility of guided local search: sample tours from it and reinforce
 * what the good samples share.  The reference has no counterpart.  Definition (the contract; gnngls_amd.host.aco restates it in
 * NumPy, bit for bit).  Per instance: D [n,n] fp64 the costs; H [n,n] fp64 the heuristic, larger = more attractive (the
 * diagonal is never read as a candidate); tau [n,n] fp64 the pheromone, IN/OUT; best_tour [n+1] int32 and best_cost fp64, IN/OUT
 * (best_cost = +inf: no tour yet; with a finite best_cost the tour's entries must be node ids).  Every fp64 operation is one add,
 * multiply or divide, rounded once.  For t = 0 .. iters-1, with the global index g = iter0 + t:
 *   1. Walks.  Ant a = 0 .. ants-1 starts at s = (a + g) mod n if spread_starts, else at node 0, and runs the walk of
 *      gnngls_sample_nn_tours with depot s and invert = 0 on the weights w_j = tau[i,j] * H[i,j] (one multiply per candidate, formed
 *      when row i is read): the same candidate order, inf rule, all-zero rule, refusal rule, summation order, x = u * total and
 *      pick rule.  Uniforms: the caller's u[b,t,a,:], or Philox4x32-10 under the same key and 53-bit formula with counter
 *      (b, g * ants + a, step, 2) -- counter word 3 = 2 keeps the stream apart from the walks' (0) and the kicks' (1).
 *   2. Cost.  The closed walk is rotated so that node 0 is first and last, direction kept; its cost is the sum gnngls_tour_cost
 *      computes for that rotated tour, in the same order (so gnngls_tour_cost of best_tour reproduces best_cost bit for bit).
 *   3. Early end.  If any walk of the iteration met refused weights, any ant's cost is not finite, or the smallest cost is not
 *      > 0, the instance's run ends here: status = GNNGLS_SAMPLE_BAD_WEIGHTS, iters_done = t, tau and the best pair as iteration
 *      t-1 left them, trace_cost[t..] untouched.  Other instances are unaffected.
 *   4. Selection.  ib = the lowest ant index among the minimal costs; trace_cost[t] = cost[ib]; the best pair is replaced only if
 *      cost[ib] < best_cost.
 *   5. Update.  The deposit tour X is the best tour so far if gb_every > 0 and (g + 1) % gb_every == 0, else ant ib's tour, and
 *      cost(X) the cost held with it.  q = 1.0 / cost(X); keep = 1.0 - rho; tau_max = 1.0 / (rho * best_cost) with the best cost
 *      after step 4; tau_min = tau_max * min_ratio.  For every ordered pair i != j: v = tau[i,j] * keep; if {i,j} is an edge of
 *      X: v = v + q; if v < tau_min: v = tau_min; if v > tau_max: v = tau_max; tau[i,j] = v.  The diagonal is never written.  The
 *      update is entry-wise (no reduction order), and a symmetric tau stays bitwise symmetric.
 * After the loop iters_done = iters and status = 0.  Chaining: K1 iterations, then K2 with iter0 = K1 fed with the first run's
 * tau, best_tour and best_cost, is the run of K1 + K2 iterations, bit for bit.
 *   D, H, tau [B,n,n]; best_tour [B,n+1]; best_cost [B]; u [B,iters,ants,n-1] or NULL; iters_done, status [B] int32;
 *   trace_cost [B,iters] or NULL; ant_tours [B,ants,n+1] int32 and ant_cost [B,ants] fp64, both or neither: the rotated tours and
 *   costs of the ants of the last iteration whose walks ran (an early-ended one included; an ant that met refused weights has a
 *   row of -1 and the cost NaN), untouched when iters = 0.
 * One workgroup of min(ants, 16) wavefronts per instance runs all iterations of the launch; ant a walks on wavefront a % 16.
 * 3 <= n <= GNNGLS_ACO_MAX_N, 1 <= ants <= GNNGLS_ACO_MAX_ANTS (beyond: GNNGLS_ERR_UNSUPPORTED); B >= 1, iters >= 0, iter0 >= 0,
 * 0 < rho < 1, 0 < min_ratio <= 1, gb_every >= 0, (iter0 + iters) * ants < 2^32, no NULL pointer other than u, trace_cost and the
 * ant pair (GNNGLS_ERR_ARG): rejected on the host, with a message, before any device work. */
#define GNNGLS_ACO_MAX_N 1024
#define GNNGLS_ACO_MAX_ANTS 256
int gnngls_aco_run(const double *D, const double *H, double *tau, int32_t *best_tour, double *best_cost, int B, int n, int ants, int iters,
                   int64_t iter0, double rho, double min_ratio, int gb_every, int spread_starts, uint64_t seed, const double *u,
                   int32_t *iters_done, int32_t *status, double *trace_cost, int32_t *ant_tours, double *ant_cost, void *stream);

/* ---- beam search: decode tours from any edge score ---------------------------------------------------------------------------
 * The most common use of a learned edge score in GNN-for-TSP work: build a tour from the score directly, greedily (width 1) or
 * keeping the `width` best partial paths.  The reference has no counterpart (its paper compares against these decoders).
 * Definition (the contract; gnngls_amd.host.beam_search restates it in NumPy, bit for bit).  Per instance: S [n,n] fp64 a
 * cost-like score, smaller = better (distances, alpha, regret predictions, -log p); optionally D [n,n] fp64 the distances.
 *   State.  A beam is a path from `depot` with a score c; beams are ordered by rank k = 0, 1, ...  Step 0: one beam, [depot],
 *      c = 0.0.
 *   Step t = 1 .. n-1.  The candidates are all pairs (beam k, node j not on beam k's path) with key = c_k + S[last_k, j]: one
 *      fp64 add, rounded once, and a key that is zero is taken as +0.0.  The new beams are the min(width, #candidates) candidates
 *      smallest in the total order (key, k, j) -- keys compare as fp64 values, ties go to the lower k, then to the lower j --
 *      ranked in that order, with c := key.  Nothing is deduplicated: two beams may hold the same node set.
 *   Close.  Every final beam gets score = c + S[last, depot] (a zero again taken as +0.0) and the tour path + [depot].  n_beams is
 *      the number of final beams; it is below width only where the tree has fewer leaves.  Given D, a beam's cost is what
 *      gnngls_tour_cost computes for its tour, in the same order and with the same bits.
 *   Select.  GNNGLS_BEAM_SELECT_SCORE: the final beam smallest in (score, rank).  GNNGLS_BEAM_SELECT_COST: the one smallest in
 *      (cost, rank), the "shortest tour" decoder; it requires D (a NaN cost leaves the choice unspecified).
 *   Refusal.  If any off-diagonal entry of S[b] is NaN or infinite, instance b gets status GNNGLS_BEAM_BAD_SCORE, n_beams = 0,
 *      tours of -1 and NaN scores and costs; other instances are unaffected.  The diagonal is never read.
 * Consequences: with width = 1 and scores whose partial sums are exact the tour is gnngls_nearest_neighbor's; with
 * width >= (n-1)! the search is exhaustive and best_score is the minimum over all tours of the left-to-right summed score.
 *   S [B,n,n]; D [B,n,n] or NULL; best_tour [B,n+1] int32; best_score, best_cost [B] fp64 (best_cost NaN without D); n_beams,
 *   status [B] int32; beam_tours [B,width,n+1] int32, beam_score and beam_cost [B,width] fp64, all three or none: every final beam
 *   by rank, rows from n_beams on -1 / NaN; workspace: device scratch of at least gnngls_beam_search_workspace_bytes(B, n, width)
 *   bytes, 16-byte aligned (the back-pointers of every step, a tour buffer and, where they do not fit into LDS, the visited bits).
 * One workgroup of min(width, 16) wavefronts per instance runs every step, the close and the selection in one launch.
 * 3 <= n <= GNNGLS_BEAM_MAX_N and 1 <= width <= GNNGLS_BEAM_MAX_WIDTH (above: GNNGLS_ERR_UNSUPPORTED); B >= 1, 0 <= depot < n,
 * select one of the two, D given for GNNGLS_BEAM_SELECT_COST, no NULL pointer other than D and the beam triple, a workspace
 * large enough (GNNGLS_ERR_ARG): rejected on the host, with a message, before any device work. */
#define GNNGLS_BEAM_MAX_N 1024
#define GNNGLS_BEAM_MAX_WIDTH 1024
#define GNNGLS_BEAM_SELECT_SCORE 0
#define GNNGLS_BEAM_SELECT_COST 1
#define GNNGLS_BEAM_BAD_SCORE 1
int64_t gnngls_beam_search_workspace_bytes(int B, int n, int width);          /* 0 for arguments out of range */
int gnngls_beam_search(const double *S, const double *D, int B, int n, int width, int depot, int select, int32_t *best_tour,
                       double *best_score, double *best_cost, int32_t *n_beams, int32_t *status, int32_t *beam_tours,
                       double *beam_score, double *beam_cost, void *workspace, int64_t workspace_bytes, void *stream);

/* ---- greedy edge matching ("greedy merge"): decode tours from any edge score ---------------------------------------------------
 * The other standard decoder of an edge score beside beam search, and the classical greedy constructor beside nearest neighbour
 * and the insertions: it looks at all edges at once instead of growing one path from the depot.  The reference has no counterpart.
 * Definition (the contract; gnngls_amd.host.greedy_edge restates it in NumPy, bit for bit).  Per instance: S [n,n] fp64 a
 * cost-like score, smaller = better; optionally D [n,n] fp64 the distances.
 *   Keys.  The key of the undirected edge {i, j}, i < j, is S[i, j] -- only the upper triangle defines it -- with -0.0 and +0.0 one
 *      key.  The edges are ordered by (key, i, j): keys compare as fp64 values, ties go to the lower i, then to the lower j.
 *   Acceptance.  Walk the edges in that order.  Every node starts with degree 0 as a path fragment of its own.  {i, j} is accepted
 *      iff deg[i] < 2, deg[j] < 2 and i and j are not the two ends of one path fragment (it would close a subtour); it joins the
 *      two fragments.  After n - 1 acceptances one Hamiltonian path is left; its two nodes of degree 1 are joined.  This closing
 *      edge is the n-th edge.
 *   Outputs.  tour [n+1]: tour[0] = tour[n] = depot, tour[1] the smaller-numbered of the depot's two tour neighbours.  score: the
 *      left-to-right sum of the keys of the edges along tour, started from 0.0; cost: the sum of D[tour[p], tour[p+1]] in the same
 *      order, as gnngls_tour_cost computes it, NaN without D.  edges [n,2] (optional): the n - 1 accepted edges as (i, j), i < j, in
 *      acceptance order, then the closing edge (smaller end first).
 *   Rounds.  The device runs the exact parallel form (gnngls_amd.host.greedy_edge_rounds restates it; DESIGN.md has the proof that
 *      it accepts the same edges).  cand[u] of a node of degree < 2 is the smallest edge {u, j} in (key, i, j) with deg[j] < 2, j not
 *      u and j not the far end of u's fragment; an edge e = {u, v} is dominant iff it is the smaller of the candidates of the two
 *      ends of u's fragment and also of v's; a round accepts all dominant edges at once.  rounds is the number of rounds until
 *      n - 1 edges are accepted: 1 <= rounds <= n - 1, a property of S alone.
 *   Refusal.  If any off-diagonal entry of S[b] is NaN or infinite, instance b gets status GNNGLS_GREEDY_EDGE_BAD_SCORE, tour and
 *      edges of -1, NaN score and cost, rounds 0; other instances are unaffected.  The diagonal is never used.
 *   What is read.  Off the diagonal every entry of S is read (the refusal), and node u's candidates are taken from ROW u: S has
 *      to be bitwise symmetric off the diagonal, which the caller guarantees (gnngls_amd.ops.greedy_edge checks it).  For a matrix
 *      that is not, the result is unspecified but bounded: valid memory only, at most n - 1 rounds, and where a round finds no
 *      dominant edge the instance ends with status GNNGLS_GREEDY_EDGE_STALLED and the outputs of a refusal.  D is read along the
 *      tour only, D[tour[p], tour[p+1]].
 *   S [B,n,n]; D [B,n,n] or NULL; tour [B,n+1] int32; score, cost [B] fp64; edges [B,n,2] int32 or NULL; rounds, status [B] int32.
 * One workgroup of min(ceil(n / 16), 16) wavefronts per instance runs the whole decode in one launch; no workspace.
 * 3 <= n <= GNNGLS_GREEDY_EDGE_MAX_N, B >= 1, 0 <= depot < n, no NULL pointer other than D and edges (GNNGLS_ERR_ARG): rejected on
 * the host, with a message, before any device work. */
#define GNNGLS_GREEDY_EDGE_MAX_N 1024
#define GNNGLS_GREEDY_EDGE_BAD_SCORE 1
#define GNNGLS_GREEDY_EDGE_STALLED 2
int gnngls_greedy_edge(const double *S, const double *D, int B, int n, int depot, int32_t *tour, double *score, double *cost,
                       int32_t *edges, int32_t *rounds, int32_t *status, void *stream);

/* Host-side query (oracle/one_tree.c has no counterpart; scripts/bench_bounds.py reports it): the launch gnngls_one_tree_bound makes
 * for n nodes -- *threads workgroup size (64 = one wavefront per instance, n <= 256), *lds_bytes dynamic LDS per workgroup,
 * *nodes_per_lane register slots per lane.  Any output pointer may be NULL. */
int gnngls_one_tree_bound_describe(int n, int *threads, int *lds_bytes, int *nodes_per_lane);

/* ---- K3: guided_local_search (algorithms.py:135-195), local_search (algorithms.py:111-132) -----
 * One persistent workgroup per instance.
 *   D            [B,n,n] fp64, symmetric (it comes from nx.attr_matrix of an undirected graph) unless
 *                penalty_bits == -1
 *   guides       [n_guides,B,n,n] fp64 utility numerators G.edges[e][guide] (algorithms.py:155),
 *                cycled per outer iteration (algorithms.py:147); may be NULL iff max_outer_iters == 0
 *   init_tour    [B,n+1], init_cost [B]
 *   max_outer_iters >= 0 : run exactly this many outer iterations (deterministic / parity mode);
 *                          0 = local_search only (algorithms.py:142)
 *   max_outer_iters <  0 : run until time_limit_s seconds of device wall clock have elapsed since
 *                          the workgroup started (reference mode, `while time.time() < t_lim`)
 *   penalty_bits width of the LDS-resident penalty counters (algorithms.py:138,161): 32, 16, or
 *                0 = auto: the fastest store that keeps all B instances resident (32-bit LDS counters, then the
 *                compact store with 32-bit counters in global memory), else the one with the largest
 *                residency.  16 = uint16 LDS counters (n=100: 3 workgroups per CU): a counter about to
 *                overflow stops that instance with GNNGLS_STATUS_PENALTY_OVERFLOW; the caller reruns it with 32.
 *                -1 = force the global-memory store: matrices stay in HBM/L2 and every evaluation keeps the
 *                reference's exact index order, so D may be ASYMMETRIC (the LDS stores keep one triangle).
 *                -2 = force the compact store (distance triangle in LDS, 32-bit counters in global memory; n <= 255).
 *   watchdog_s   hard abort (status GNNGLS_STATUS_WATCHDOG) if a workgroup runs longer than this
 *   outputs      best_tour [B,n+1], best_cost [B], outer_iters [B] (int64),
 *                trace_cost [B,trace_cap] cost after every accepted move (algorithms.py:127-130,
 *                180-183), trace_time [B,trace_cap] seconds since workgroup start (optional),
 *                trace_len [B] = number of accepted moves (may exceed trace_cap),
 *                penalty_out [B,n,n] int32 final penalties (optional),
 *                evals_out [B] int64 number of delta evaluations (optional), status [B] (optional)
 *   improvement trace (optional, any of the arrays may be NULL; imp_len == NULL disables it): one entry whenever the
 *                returned best improves -- after the initial descent (algorithms.py:143) and after an outer
 *                iteration whose descent ends below the best so far (algorithms.py:190-191):
 *                imp_cost [B,imp_cap] the new best cost, imp_time [B,imp_cap] seconds since workgroup start,
 *                imp_iter [B,imp_cap] int64 number of completed outer iterations (0 = initial descent),
 *                followed by ONE terminal entry (best_cost[b], time at the end of the search, outer_iters[b]);
 *                imp_len [B] = improvements + 1 (may exceed imp_cap: the terminal entry then takes the last slot, so
 *                with imp_cap >= 1 entry min(imp_len, imp_cap) - 1 is always the terminal one).
 *                A 10 s TSP100 search accepts ~2e6 moves but improves its best a few dozen times: this is the
 *                search-progress record (test.py:97-117, `best_cost` = cummin) that stays bounded at any run length;
 *                the per-move trace is exact while trace_len[b] <= trace_cap and TRUNCATED beyond (callers must check).
 * If trace_cap == 0 the per-move tour_cost recomputation (algorithms.py:176) is deferred to the
 * end of each perturbation phase -- the values that drive decisions are unchanged. */
int gnngls_gls_run(const double *D, const double *guides, int n_guides, int B, int n,
                   const int32_t *init_tour, const double *init_cost,
                   int perturbation_moves, int first_improvement, int penalty_bits,
                   int64_t max_outer_iters, double time_limit_s, double watchdog_s,
                   int32_t *best_tour, double *best_cost, int64_t *outer_iters,
                   double *trace_cost, float *trace_time, int trace_cap, int32_t *trace_len,
                   int32_t *penalty_out, int64_t *evals_out, int32_t *status,
                   double *imp_cost, float *imp_time, int64_t *imp_iter, int imp_cap, int32_t *imp_len, void *stream);

/* ---- regret labels of the training data: datasets.set_labels (datasets.py:23-34) ----------------------------------------
 * The reference labels every edge e outside the optimal tour with regret = (cost - opt) / opt, cost = tour_cost of the tour
 * fixed_edge_tour (gnngls/__init__.py:63-79) returns: LKH with e forced into the tour.  Here that constrained solve is a
 * FIXED-EDGE SEARCH: the reference's guided_local_search (algorithms.py:135-195) on the instance with one changed weight,
 *     w'(i,j) = w'(j,i) = fl(D[i,j] - M_b),   M_b = the smallest power of two >= (2.0 n) * max(D_b)   (frexp / ldexp: exact),
 * guides = ['weight'] on that matrix D' (the fixed edge has a negative utility and is never penalised), started from the base
 * tour (which does not hold the edge), for exactly max_outer_iters outer iterations.  Every tour with the edge costs less under
 * D' than every tour without it, and the first descent inserts it (a relocate move next to i is worth about -M), so the
 * returned best tour holds the edge; its label is its TRUE cost (tour_cost on D, gnngls/__init__.py:17-21).
 *   D            [B,n,n] fp64, bitwise symmetric (else GNNGLS_ERR_ARG); 3 <= n <= 255
 *   base_tour    [B,n+1] a tour from depot 0 per instance (the reference's optimal tour; here the best tour known)
 *   edge_mask    [B,N] uint8 or NULL.  NULL: every edge off the base tour gets a search; edge_cost is output only.
 *                Else only the masked edges off the base tour get one, and edge_cost is IN/OUT: the results are min-merged into
 *                it (the repair rounds of gnngls_amd.labels: costs of earlier calls are true costs of real tours with the edge)
 *   perturbation_moves, max_outer_iters (>= 0), penalty_bits, watchdog_s: as gnngls_gls_run, per search; searches that end with
 *                GNNGLS_STATUS_PENALTY_OVERFLOW are rerun with 32-bit counters
 *   chunk_jobs   searches per launch of the search kernel (0 = gnngls_regret_labels_chunk(n)); each holds its own D' [n,n] in
 *                stream-ordered workspace.  Results do not depend on it.
 *   outputs      edge_cost [B,N]: base edges = the base tour's cost, other edges = min over the results they received;
 *                regret [B,N] = (edge_cost - base_cost) / base_cost (datasets.py:31), exactly 0.0 on base edges -- NEGATIVE where a
 *                search found a tour cheaper than the base (the caller then repairs the base, gnngls_amd.labels.regret_labels);
 *                best_tour [B,n+1], best_cost [B]: the cheapest tour seen (the base or a search result; ties -> the base, then the
 *                lowest edge index); status [B]: the most severe search status (GNNGLS_STATUS_WATCHDOG, GNNGLS_STATUS_EDGE_LOST)
 * Bad arguments are rejected on the host before any device work.  The call synchronises the stream once per chunk (the host
 * builds the job lists and reads the search statuses). */
int gnngls_regret_labels_chunk(int n);
int gnngls_regret_labels(const double *D, int B, int n, const int32_t *base_tour, const uint8_t *edge_mask,
                         int perturbation_moves, int64_t max_outer_iters, int penalty_bits, double watchdog_s, int chunk_jobs,
                         double *edge_cost, double *regret, int32_t *best_tour, double *best_cost, int32_t *status, void *stream);

/* ---- K1/K2: edge-regret GNN forward ------------------------------------------------------------
 * EdgePropertyPredictionModel.forward (models.py:44-70) on the line graph of K_n (datasets.py:56-60),
 * specialised to the reference architecture: embed_dim 128, 8 heads x 16 (GATConv(128,16,8),
 * models.py:23), MLP hidden 512 (models.py:60), out_dim 1, eval-mode BatchNorm.  Layer count is a
 * run-time argument (the reference builds n_heads layers, models.py:59-61).
 *
 * Packed fp32 weight image (all blocks 16-byte aligned), in this order:
 *   embed_w[128*in_dim] embed_b[128]
 *   per layer: fc_w[128*128] attn_l[128] attn_r[128] bn1_scale[128] bn1_shift[128]
 *              w1[512*128] b1[512] w2[128*512] b2[128] bn2_scale[128] bn2_shift[128]
 *   dec_w[128] dec_b[1] pad[3]
 * where bn_scale = gamma / sqrt(running_var + eps), bn_shift = beta - running_mean * bn_scale
 * (eval-mode BatchNorm1d, models.py:28,35).  gnngls_amd.models packs a reference state_dict.
 *
 *   feat [B,N,in_dim] fp32 scaled edge features in line-graph node order (node = rank of (i<j) in
 *        itertools.combinations order); y_out [B,N] fp32.
 *   workspace: device scratch of at least gnngls_regret_forward_workspace_bytes(1, n) bytes; if it
 *        is smaller than the full-batch size the batch is processed in instance chunks. */
#define GNNGLS_MODEL_EMBED_DIM 128
#define GNNGLS_MODEL_HEADS 8
#define GNNGLS_MODEL_HIDDEN 512
int64_t gnngls_model_packed_floats(int in_dim, int n_layers);
int64_t gnngls_regret_forward_workspace_bytes(int B, int n);
int gnngls_regret_forward(const float *feat, const float *weights, int B, int n, int in_dim, int n_layers,
                          float *y_out, void *workspace, int64_t workspace_bytes, void *stream);

/* ABI v4 -- the same forward with the weight-only work hoisted out of it (test.py:43-54 loads a checkpoint ONCE and then
 * calls the model per instance, test.py:72-77): the feed-forward block (models.py:26-36) and the folded GATConv fc (models.py:23)
 * run on the bf16 matrix pipe from three bf16 pieces per fp32 weight in MFMA fragment order; that image depends on the weights
 * only.  gnngls_regret_prepare writes it for all layers into `prepared` (caller-owned device memory of
 * gnngls_regret_prepared_bytes(n_layers) bytes, valid until the weights change); gnngls_regret_forward_prepared is
 * gnngls_regret_forward reading it (prepared == NULL: the feed-forward block stays on the fp32 matrix pipe).
 * The image also holds A = We^T Wfc0^T [in_dim,128] and b' = Wfc0 be: the embedding (models.py:57,66) and the first layer's fc
 * (models.py:23) are both linear in the in_dim input features, so with an image (in_dim <= 32) ft = x A + b' is written by the
 * embedding pass itself instead of a [B N,128] x [128,128] product.
 * gnngls_regret_forward itself prepares into stream-ordered scratch on every call (2 launches per layer more). */
int64_t gnngls_regret_prepared_bytes(int n_layers);
int gnngls_regret_prepare(const float *weights, int in_dim, int n_layers, void *prepared, int64_t prepared_bytes, void *stream);
int gnngls_regret_forward_prepared(const float *feat, const float *weights, const void *prepared, int64_t prepared_bytes,
                                   int B, int n, int in_dim, int n_layers,
                                   float *y_out, void *workspace, int64_t workspace_bytes, void *stream);

/* ---- N4: one training step of the same model (scripts/train.py:20-32) -------------------------------------------
 * model.train(); y_pred = model(batch, x); loss = criterion(y_pred, y); loss.backward() for a dgl.batch of B line graphs
 * of K_n (train.py:118-121): BatchNorm1d uses the statistics of all B*N rows (models.py:27,35), GATConv is
 * differentiated through its edge softmax (models.py:23).  The criterion itself (MSELoss / BCEWithLogitsLoss,
 * train.py:106-112) is elementwise on [B*N] values and stays with the caller: the forward returns y_pred, the backward
 * takes dy = d loss / d y_pred.
 *
 * `params` is the RAW parameter image: the layout of the packed inference image above with the BatchNorm slots holding
 * gamma / beta instead of the folded scale / shift (gnngls_model_packed_floats floats); `grads` has the same layout.
 *   forward : feat [B,N,in_dim] -> y_out [B,N]; bn_batch_stats [n_layers][2 (BN1, BN2)][2 (mean, unbiased var)][128]
 *             is what the caller folds into running_mean / running_var (momentum update, torch semantics).
 *   backward: must follow a forward on the SAME workspace (activations are kept there); writes every gradient.
 * n <= 257 (register-resident source tiles of the attention backward: instantiations for n <= 145, <= 209, <= 257).
 * A GATConv bias (DGL >= 0.7 checkpoints) is not part of the image: in training mode BatchNorm-1's batch mean absorbs
 * it (prediction unchanged, gradient exactly zero); the caller adds it to the BatchNorm-1 batch mean it folds into
 * running_mean (gnngls_amd/models.py:_TrainStep does). */
int64_t gnngls_regret_train_workspace_bytes(int B, int n, int n_layers);
int gnngls_regret_train_forward(const float *feat, const float *params, int B, int n, int in_dim, int n_layers, float bn_eps,
                                float *y_out, float *bn_batch_stats, void *workspace, int64_t workspace_bytes, void *stream);
int gnngls_regret_train_backward(const float *feat, const float *params, const float *dy, int B, int n, int in_dim,
                                 int n_layers, float *grads, void *workspace, int64_t workspace_bytes, void *stream);

/* ---- other head counts: GATConv(128, 128 / n_heads, n_heads) (models.py:23) with n_heads layers (models.py:59-61) ----------
 * The reference builds any head count that divides embed_dim (scripts/train.py:76 --n_heads); with embed_dim 128 these entries
 * take n_heads in {1, 2, 4, 8, 16} (F = 128 / n_heads features per head).  The weight images keep their size and layout for every
 * head count (attn_l / attn_r hold the (1, n_heads, F) parameters flattened head-major: 128 floats), so
 * gnngls_model_packed_floats and gnngls_regret_prepared_bytes hold as they are.  Each entry below is the entry without the
 * _heads suffix with `n_heads` next to n_layers; n_heads = 8 IS that entry (same kernels, same results).  Any other n_heads
 * returns GNNGLS_ERR_UNSUPPORTED before any device work.  Limits for n_heads != 8: 3 <= n <= 257 in the forward and the
 * training step (the 8-head forward goes to n = 423); a larger n returns GNNGLS_ERR_UNSUPPORTED.
 * The prepared image does not depend on the head count (its rank-1 first-layer coefficients are read by the 8-head forward
 * only), so an image made by either prepare entry is valid for every head count of the same weights. */
int gnngls_model_heads_supported(int n_heads);                          /* 1 for n_heads in {1, 2, 4, 8, 16}, else 0 */
int64_t gnngls_regret_forward_workspace_bytes_heads(int B, int n, int n_heads);         /* 16 heads: 256 B per node more */
int gnngls_regret_forward_heads(const float *feat, const float *weights, int B, int n, int in_dim, int n_layers, int n_heads,
                                float *y_out, void *workspace, int64_t workspace_bytes, void *stream);
int gnngls_regret_prepare_heads(const float *weights, int in_dim, int n_layers, int n_heads, void *prepared, int64_t prepared_bytes,
                                void *stream);
int gnngls_regret_forward_prepared_heads(const float *feat, const float *weights, const void *prepared, int64_t prepared_bytes,
                                         int B, int n, int in_dim, int n_layers, int n_heads,
                                         float *y_out, void *workspace, int64_t workspace_bytes, void *stream);
/* training step (scripts/train.py:20-32); the workspace of 16 heads keeps per-head softmax statistics (2 x 16 per node) */
int64_t gnngls_regret_train_workspace_bytes_heads(int B, int n, int n_layers, int n_heads);
int gnngls_regret_train_forward_heads(const float *feat, const float *params, int B, int n, int in_dim, int n_layers, int n_heads,
                                      float bn_eps, float *y_out, float *bn_batch_stats, void *workspace, int64_t workspace_bytes,
                                      void *stream);
int gnngls_regret_train_backward_heads(const float *feat, const float *params, const float *dy, int B, int n, int in_dim,
                                       int n_layers, int n_heads, float *grads, void *workspace, int64_t workspace_bytes,
                                       void *stream);

/* get_scaled_features (datasets.py:73-95) for features=[weight] (datasets.py:14-20):
 * feat[b, rank(i<j)] = MinMaxScaler.transform(float32(D[b,i,j])) with sklearn's fp32 arithmetic
 * (x*scale_ rounded to fp32, + min_ rounded to fp32). */
int gnngls_pack_features(const double *D, int B, int n, double scale, double min_, float *feat, void *stream);

/* test.py:79-83: regret_pred = max(MinMaxScaler.inverse_transform(y_pred), 0) as a symmetric fp64
 * [B,n,n] matrix (zero diagonal) -- the 'regret_pred' guide of guided_local_search. */
int gnngls_unpack_regret(const float *y, int B, int n, double scale, double min_, double *out, void *stream);

/* Test hook: lowers the value at which a 16-bit penalty counter reports overflow (default 65535) so
 * the overflow -> rerun-with-32-bit path can be exercised in seconds.  Never called by the product. */
int gnngls_debug_set_penalty16_limit(int limit);

/* Experiment hook: forces the workgroup size of gnngls_gls_run (64, 128, 256 or 512 threads; 0 = the default policy by
 * instance size).  Used by scripts/probe_gls.py to measure the policy; never called by the product. */
int gnngls_debug_set_gls_threads(int threads);

/* Register budget of the kernel instantiation gnngls_gls_run would launch for (n, B, penalty_bits), as resident wavefronts
 * per SIMD: 4 = the 128-VGPR builds (no scratch), 2 = the 256-VGPR build of the single-wavefront kernel (n = 8 .. 33, at
 * most 2048 instances: TSP20 x 1000; no scratch) -- every BASELINE.json shape runs on these two --, 6 / 8 = the 80- / 64-VGPR
 * builds (56-148 B of scratch per lane) that only batches of small instances beyond 16 workgroups per CU select
 * (e.g. TSP20 x 5000).  0 = bad argument. */
int gnngls_gls_waves_per_simd(int n, int B, int penalty_bits);

/* 1 if gnngls_gls_run would run the perturbation phase of this (n, B, penalty_bits) on ALL wavefronts of the workgroup
 * (the "team" form: the four one-to-all scans of a penalty step, algorithms.py:167-174, evaluated concurrently and consumed
 * in the reference's order), 0 if on wavefront 0 only.  Since round 5 the policy picks it for FIRST-IMPROVEMENT runs only
 * (16-wave workgroups that own a CU by their LDS footprint -- compact store, n >= 144: TSP200 -- when B <= number of CUs):
 * for best-improvement runs the edge form of the serial phase is faster there too, so this query (a best-improvement
 * answer) returns 0 unless the test hook below forces the form; gnngls_gls_describe_run reports a first-improvement launch.
 * Same results either way (bit-exact); this only reports the policy. */
int gnngls_gls_uses_team(int n, int B, int penalty_bits);

/* Experiment / test hook: -1 = the policy above (default), 0 = never use the team form, 1 = use it wherever it exists
 * (symmetric stores with 32-bit counters, n <= 255) whatever the batch size.  Never called by the product. */
int gnngls_debug_set_gls_team(int mode);

/* Experiment / test hook: 0 = the descent (algorithms.py:111-132) evaluates every move of an all-to-all scan; -1 / 1
 * (default) = the pruned scans where they exist (best improvement, symmetric LDS stores, max |D| <= 1e6; the 2-opt scan from
 * n = 80, the relocate scan from n = 128): per
 * node a list of its 32 nearest nodes, only moves that can qualify are evaluated -- a superset of the qualifying moves,
 * hence the same arg-min, bit-exact.  Never called by the product. */
int gnngls_debug_set_gls_prune(int mode);

/* Diagnostic hook: device buffer of 16 int64 per instance that a library built with -DGLS_STAMPS fills with
 * per-phase shader-cycle totals of gnngls_gls_run (scripts/probe_gls_stamps.py).  Ignored by normal builds. */
int gnngls_debug_set_stamp_buffer(void *device_buffer);

/* ---- measurement hooks (bench.py): per-kernel-class device time via HIP events recorded on the
 * caller's stream around every launch made while profiling is enabled.  gnngls_profile_collect
 * synchronises the recorded events, sums milliseconds and launch counts per class (arrays of
 * GNNGLS_PROF_KINDS entries) and clears the log. */
enum {
    GNNGLS_PROF_PACK = 0, GNNGLS_PROF_EMBED, GNNGLS_PROF_GEMM_FC, GNNGLS_PROF_GAT_ROWS, GNNGLS_PROF_GAT_ROWS_RANK1 /* (the slot of the retired gat_combine) */,
    GNNGLS_PROF_GEMM_FFN1, GNNGLS_PROF_GEMM_FFN2, GNNGLS_PROF_DECISION, GNNGLS_PROF_UNPACK,
    GNNGLS_PROF_NEAREST_NEIGHBOR, GNNGLS_PROF_TOUR_COST, GNNGLS_PROF_GLS, GNNGLS_PROF_FFN_FUSED,
    GNNGLS_PROF_TRAIN_COLSUM, GNNGLS_PROF_TRAIN_ELEMENTWISE, GNNGLS_PROF_TRAIN_GEMM_BWD, GNNGLS_PROF_TRAIN_GEMM_TN,
    GNNGLS_PROF_TRAIN_GAT_BWD, GNNGLS_PROF_INSERTION /* gnngls_insertion and gnngls_cheapest_insertion */, GNNGLS_PROF_ONE_TREE_BOUND, GNNGLS_PROF_KINDS
};
int gnngls_profile_enable(int on);
int gnngls_profile_collect(double *ms_by_kind, int64_t *launches_by_kind);

/* Measurement hook (bench.py): while a device buffer is set (NULL = off, the default), every gnngls_gls_run launch fills its
 * first B int64 entries with the number of delta evaluations the kernel actually EXECUTED per instance.
 * evals_out of gnngls_gls_run counts what the reference evaluates (operators.py:36-39,133-136: every move of every scan);
 * the pruned descent scans (n >= 80) evaluate only the moves that can qualify, the full scans and the one-to-all scans of
 * the perturbation phase every move once -- so executed <= evals_out, equal where nothing is pruned.  Counting costs the
 * pruned scans 2-3 % (profiles/r04_ab_exec_counter.log), so it lives in kernel instantiations of their own that ONLY a
 * launch with this hook set selects: compact store (penalty_bits 0 / -2 where that store is picked), best improvement, no
 * per-move trace.  A pruning run on any other configuration reports -1 per instance.
 * ABI v3: the buffer holds 5 x B int64 -- [0, B) the counts above, then four records of the same launch for bench.py's
 * critical-path figure (written by the counting instantiations, else 0): [B, 2B) shader cycles of the instance's workgroup,
 * [2B, 3B) shader cycles of its serial perturbation phase (algorithms.py:150-185, wavefront 0), [3B, 4B) penalty steps of
 * that phase (edge form), [4B, 5B) 100 MHz device-clock ticks of the workgroup.
 * ABI v4: GNNGLS_EXEC_RECORDS = 16 records of B int64 -- after the five above the cycle account of the descent of the outer
 * iterations (algorithms.py:188 -> 111-132; wavefront 0 of the workgroup): [5B, 6B) shader cycles in local_search, then count and
 * cycles of the two_opt_a2a scans [6B, 8B), of the relocate_a2a scans evaluated in full [8B, 10B) and over the flagged rows only
 * [10B, 12B) (operators.py:32-50,129-147), [12B, 13B) cycles of the workgroup arg-min incl. waiting for the slowest wavefront,
 * [13B, 14B) of move application + barrier (algorithms.py:122-126), [14B, 15B) accepted moves, [15B, 16B) reserved.
 * The buffer must hold GNNGLS_EXEC_RECORDS x the largest B launched while it is set; process-wide, not per stream. */
#define GNNGLS_EXEC_RECORDS 16
int gnngls_profile_set_executed_evals(int64_t *device_buffer);

#ifdef __cplusplus
}
#endif
#endif /* GNNGLS_HIP_H */
