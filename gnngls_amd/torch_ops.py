"""PyTorch-ROCm custom operators of the hot path: `torch.ops.gnngls.*` (north_star).

Ten operators and, since the Or-opt descent, iterated local search, the 3-opt descent and guided local search over Or-opt, an
eleventh to a fourteenth, with the ant system a fifteenth, with beam search a sixteenth and with greedy edge
matching a seventeenth, are registered with
`torch.library` over the C ABI of libgnngls_hip.so (include/gnngls_hip.h).  Each has
exactly ONE implementation, for the CUDA dispatch key (= HIP on ROCm): there is no CPU kernel behind any of them, so
calling one with CPU tensors fails in the dispatcher ("no CPU fallback" is structural, not a runtime check).  Shape
functions (fake/meta kernels) are registered so the ops can be traced and used under FakeTensorMode.  All ops enqueue on
the current HIP stream, take caller-owned contiguous tensors and retain nothing.

    regret_forward(feat[B,N] f32, packed_weights f32, n, heads=8, head_dim=16, hidden=512, layers) -> [B,N] f32
        EdgePropertyPredictionModel.forward (models.py:44-70); packed_weights = model.pack_weights(device);
        (heads, head_dim) in {(1, 128), (2, 64), (4, 32), (8, 16), (16, 8)} (embed_dim 128)
    two_opt_delta_all(tour[B,n+1] i32, D[B,n,n] f64) -> [B,n+1,n+1] f64          operators.py:14-29
    relocate_delta_all(tour, D) -> [B,n+1,n+1] f64                                operators.py:83-103
    local_search(tour, cost[B] f64, D, first_improvement) -> (tour, cost, n_moves[B] i32)      algorithms.py:111-132
    gls_run(D, guides[G,B,n,n] f64, init_tour, init_cost, perturbation_moves, max_outer_iters, time_limit_s,
            first_improvement, trace_capacity) -> (best_tour, best_cost, outer_iters[B] i64, trace_cost[B,T] f64,
            trace_len[B] i32)                                                      algorithms.py:135-195
    insertion(W[B,n,n] f64, depot, mode, order[B,n-1] i32 or None) -> tour[B,n+1] i32          algorithms.py:82-108
        mode in {'nearest', 'farthest', 'random'}; 'random' takes the node order (None: drawn with np.random.choice)
    cheapest_insertion(sub_tour[B,len] i32, node[B] i32, W) -> (tour[B,len+1] i32, cost[B] f64)   algorithms.py:67-79
    one_tree_bound(D[B,n,n] f64, ub[B] f64, max_iters) -> (bound[B] f64, pi[B,n] f64, iters[B] i32, exit_kind[B] i32, status[B] i32)
        the Held-Karp 1-tree lower bound of oracle/one_tree.c (in place of Concorde's optimum, scripts/test.py:62,104)
    alpha_nearness(D[B,n,n] f64, pi[B,n] f64 or None) -> alpha[B,n,n] f64
        Helsgaun's alpha-nearness under the potentials of one_tree_bound (None: zeros): a model-free guide for gls_run
    or_opt_descent(tour, cost[B] f64, D, max_seg, reverse, max_moves, trace_cap) -> (tour, cost, n_moves[B] i32, status[B] i32,
        trace_cost[B,trace_cap] f64): local_search with Or-opt (chains of 1..max_seg nodes) in relocate's place; status 3 marks an
        instance whose matrix is not symmetric (outputs = inputs) -- the op reports, gnngls_amd.ops.or_opt_descent raises
    sample_nn_tours(W[B,n,n] f64, R, depot, invert, seed, u[B,R,n-1] f64 or None) -> (tours[B,R,n+1] i32, status[B,R] i32)
        algorithms.py:21-50, R sampled walks per instance; status 6 (and a tour of -1) marks a walk that met weights which are
        no probabilities -- the op reports, gnngls_amd.ops.sample_nn_tours raises
    ils(tour, cost[B] f64, D, kicks, kick0, max_seg, reverse, max_moves, seed, u[B,kicks,3] f64 or None) -> (tour, cost,
        n_moves[B] i32, accepted[B] i32, status[B] i32, trace_cost[B,kicks] f64): iterated local search -- or_opt_descent, then
        `kicks` double-bridge kicks each followed by the descent, the better tour kept; trace_cost = the candidate's cost after
        every kick (NaN: never ran); status 3 as for or_opt_descent -- the op reports, gnngls_amd.ops.ils raises
    three_opt_descent(tour, cost[B] f64, D, max_moves, trace_capacity) -> (tour, cost, n_moves[B] i32, status[B] i32,
        trace_cost[B,trace_capacity] f64): local_search with the exhaustive 3-opt scan in relocate's place, n <= 256; status 3 as
        for or_opt_descent -- the op reports, gnngls_amd.ops.three_opt_descent raises
    guided_or_opt(tour, cost[B] f64, D, guides[G,B,n,n] f64, outer_iters, iter0, k[B] f64 or None, penalty[B,n,n] i32 or None,
        perturbation_moves, max_seg, reverse, max_moves, max_steps, trace_capacity) -> (tour, cost, best_tour, best_cost,
        n_moves[B] i32, steps[B] i32, status[B] i32, penalty[B,n,n] i32, trace_cost[B,trace_capacity] f64, trace_len[B] i32):
        guided local search over 2-opt and Or-opt in one launch, n <= 1024 (algorithms.py:135-195 with the Or-opt scans in
        relocate's places); functional: the given penalties are copied, the counters after the run are returned; max_moves /
        max_steps <= 0 = the defaults of gnngls_amd.ops.guided_or_opt; status 3 as for or_opt_descent -- the op reports,
        gnngls_amd.ops.guided_or_opt raises
    aco(D[B,n,n] f64, H[B,n,n] f64, ants, iters, iter0, rho, min_ratio, gb_every, spread_starts, seed, u[B,iters,ants,n-1] f64 or
        None, tau[B,n,n] f64 or None, best_tour[B,n+1] i32 or None, best_cost[B] f64 or None) -> (best_tour, best_cost, tau,
        iters_done[B] i32, status[B] i32, trace_cost[B,iters] f64, ant_tours[B,ants,n+1] i32, ant_cost[B,ants] f64): a MAX-MIN ant
        system in one launch, n <= 1024, ants <= 256; functional: a given tau is copied, the pheromone after the run is returned;
        min_ratio <= 0 = 1 / (2 n); status 6 marks an instance whose run met weights that are no probabilities -- the op reports,
        gnngls_amd.ops.aco raises
    beam_search(S[B,n,n] f64, D[B,n,n] f64 or None, width, depot, select) -> (best_tour[B,n+1] i32, best_score[B] f64, best_cost[B] f64,
        n_beams[B] i32, status[B] i32, beam_tours[B,width,n+1] i32, beam_score[B,width] f64, beam_cost[B,width] f64): beam-search
        decoding from any edge score in one launch, n <= 1024, width <= 1024; select in {'score', 'cost'} ('cost' needs D);
        rows from n_beams on are -1 / NaN; status 1 marks an instance whose score has an off-diagonal entry that is not finite
        -- the op reports, gnngls_amd.ops.beam_search raises
    greedy_edge(S[B,n,n] f64, D[B,n,n] f64 or None, depot) -> (tour[B,n+1] i32, score[B] f64, cost[B] f64, edges[B,n,2] i32,
        rounds[B] i32, status[B] i32): greedy edge matching from any edge score in one launch, n <= 1024; S bitwise symmetric off
        the diagonal (not checked here); status 1 marks an instance whose score has an off-diagonal entry that is not finite
        -- the op reports, gnngls_amd.ops.greedy_edge raises
"""
import ctypes

import torch

from . import _lib, ops

_LIB = torch.library.Library("gnngls", "DEF")
_LIB.define("regret_forward(Tensor feat, Tensor packed_weights, int n, int heads, int head_dim, int hidden, int layers) -> Tensor")
_LIB.define("two_opt_delta_all(Tensor tour, Tensor D) -> Tensor")
_LIB.define("relocate_delta_all(Tensor tour, Tensor D) -> Tensor")
_LIB.define("local_search(Tensor tour, Tensor cost, Tensor D, bool first_improvement) -> (Tensor, Tensor, Tensor)")
_LIB.define("gls_run(Tensor D, Tensor guides, Tensor init_tour, Tensor init_cost, int perturbation_moves, "
            "int max_outer_iters, float time_limit_s, bool first_improvement, int trace_capacity) "
            "-> (Tensor, Tensor, Tensor, Tensor, Tensor)")
_LIB.define("insertion(Tensor W, int depot, str mode, Tensor? order) -> Tensor")
_LIB.define("cheapest_insertion(Tensor sub_tour, Tensor node, Tensor W) -> (Tensor, Tensor)")
_LIB.define("one_tree_bound(Tensor D, Tensor ub, int max_iters) -> (Tensor, Tensor, Tensor, Tensor, Tensor)")
_LIB.define("alpha_nearness(Tensor D, Tensor? pi) -> Tensor")
_LIB.define("or_opt_descent(Tensor tour, Tensor cost, Tensor D, int max_seg, bool reverse, int max_moves, int trace_cap) -> (Tensor, Tensor, Tensor, Tensor, Tensor)")
_LIB.define("sample_nn_tours(Tensor W, int R, int depot, bool invert, int seed, Tensor? u) -> (Tensor, Tensor)")
_LIB.define("ils(Tensor tour, Tensor cost, Tensor D, int kicks, int kick0, int max_seg, bool reverse, int max_moves, int seed, Tensor? u) "
            "-> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)")
_LIB.define("three_opt_descent(Tensor tour, Tensor cost, Tensor D, int max_moves, int trace_capacity) -> (Tensor, Tensor, Tensor, Tensor, Tensor)")
_LIB.define("guided_or_opt(Tensor tour, Tensor cost, Tensor D, Tensor guides, int outer_iters, int iter0, Tensor? k, Tensor? penalty, "
            "int perturbation_moves, int max_seg, bool reverse, int max_moves, int max_steps, int trace_capacity) "
            "-> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)")
_LIB.define("aco(Tensor D, Tensor H, int ants, int iters, int iter0, float rho, float min_ratio, int gb_every, bool spread_starts, int seed, "
            "Tensor? u, Tensor? tau, Tensor? best_tour, Tensor? best_cost) -> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)")
_LIB.define("beam_search(Tensor S, Tensor? D, int width, int depot, str select) -> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)")
_LIB.define("greedy_edge(Tensor S, Tensor? D, int depot) -> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)")

_workspaces = {}      # device index -> uint8 scratch tensor for the forward (grown on demand, reused across calls)


def _regret_forward(feat, packed_weights, n, heads, head_dim, hidden, layers):
    if heads not in (1, 2, 4, 8, 16) or heads * head_dim != 128 or hidden != 512:
        raise NotImplementedError("gnngls::regret_forward is specialised to embed_dim 128 = heads x head_dim with heads in "
                                  f"{{1, 2, 4, 8, 16}} and hidden 512 (models.py:23,60; got {heads} x {head_dim}, {hidden})")
    L = _lib.load()
    N = n * (n - 1) // 2
    feat = feat.contiguous().float()
    in_dim = 1 if feat.dim() == 2 else feat.shape[-1]
    B = feat.numel() // (N * in_dim)
    expect = int(L.gnngls_model_packed_floats(in_dim, layers))
    if packed_weights.numel() != expect or packed_weights.dtype != torch.float32:
        raise ValueError(f"packed_weights must hold {expect} fp32 values for in_dim={in_dim}, layers={layers}")
    if heads == 8:
        need = int(L.gnngls_regret_forward_workspace_bytes(B, n))
        ws_bytes = min(need, max(int(L.gnngls_regret_forward_workspace_bytes(1, n)), 48 << 30))
    else:
        need = int(L.gnngls_regret_forward_workspace_bytes_heads(B, n, heads))
        ws_bytes = min(need, max(int(L.gnngls_regret_forward_workspace_bytes_heads(1, n, heads)), 48 << 30))
    key = feat.device.index
    ws = _workspaces.get(key)
    if ws is None or ws.numel() < ws_bytes:
        _workspaces[key] = None
        ws = _workspaces[key] = torch.empty(ws_bytes, dtype=torch.uint8, device=feat.device)
    y = torch.empty((B, N), dtype=torch.float32, device=feat.device)
    if heads == 8:
        _lib.check(L.gnngls_regret_forward(_lib.ptr(feat), _lib.ptr(packed_weights.contiguous()), B, n, in_dim, layers, _lib.ptr(y),
                                           _lib.ptr(ws), ctypes.c_int64(ws.numel()), _lib.current_stream()), "regret_forward")
    else:
        _lib.check(L.gnngls_regret_forward_heads(_lib.ptr(feat), _lib.ptr(packed_weights.contiguous()), B, n, in_dim, layers, heads,
                                                 _lib.ptr(y), _lib.ptr(ws), ctypes.c_int64(ws.numel()), _lib.current_stream()),
                   "regret_forward")
    return y


def _local_search(tour, cost, D, first_improvement):
    r = ops.gls_run(D, None, tour, cost, first_improvement=first_improvement, max_outer_iters=0)
    return r.best_tour, r.best_cost, r.trace_len


def _gls_run(D, guides, init_tour, init_cost, perturbation_moves, max_outer_iters, time_limit_s, first_improvement,
             trace_capacity):
    r = ops.gls_run(D, guides, init_tour, init_cost, perturbation_moves=perturbation_moves,
                    first_improvement=first_improvement, max_outer_iters=max_outer_iters, time_limit_s=time_limit_s,
                    trace_cap=trace_capacity)
    trace = r.trace_cost if r.trace_cost is not None else torch.zeros((D.shape[0], 0), dtype=torch.float64, device=D.device)
    return r.best_tour, r.best_cost, r.outer_iters, trace, r.trace_len


def _one_tree_bound(D, ub, max_iters):
    r = ops.one_tree_bound(D, ub, max_iters=max_iters)
    return r.bound, r.pi, r.iters, r.exit_kind, r.status


_LIB.impl("regret_forward", _regret_forward, "CUDA")
_LIB.impl("two_opt_delta_all", ops.two_opt_delta_all, "CUDA")
_LIB.impl("relocate_delta_all", ops.relocate_delta_all, "CUDA")
_LIB.impl("local_search", _local_search, "CUDA")
_LIB.impl("gls_run", _gls_run, "CUDA")
_LIB.impl("insertion", ops.insertion, "CUDA")
_LIB.impl("cheapest_insertion", ops.cheapest_insertion, "CUDA")
_LIB.impl("one_tree_bound", _one_tree_bound, "CUDA")
_LIB.impl("alpha_nearness", ops.alpha_nearness, "CUDA")
def _or_opt_descent(tour, cost, D, max_seg, reverse, max_moves, trace_cap):
    r = ops.or_opt_launch(tour, cost, D, max_seg, reverse, max_moves, trace_cap)
    trace = r.trace_cost if r.trace_cost is not None else torch.zeros((tour.shape[0], 0), dtype=torch.float64, device=tour.device)
    return r.tour, r.cost, r.moves, r.status, trace


_LIB.impl("or_opt_descent", _or_opt_descent, "CUDA")
_LIB.impl("sample_nn_tours", ops.sample_nn_launch, "CUDA")


def _ils(tour, cost, D, kicks, kick0, max_seg, reverse, max_moves, seed, u):
    r = ops.ils_launch(tour, cost, D, kicks, max_seg, reverse, max_moves, seed, u, kick0, want_trace=True)
    return r.tour, r.cost, r.moves, r.accepted, r.status, r.trace_cost


_LIB.impl("ils", _ils, "CUDA")


def _three_opt_descent(tour, cost, D, max_moves, trace_capacity):
    r = ops.three_opt_launch(tour, cost, D, max_moves, trace_capacity)
    trace = r.trace_cost if r.trace_cost is not None else torch.zeros((tour.shape[0], 0), dtype=torch.float64, device=tour.device)
    return r.tour, r.cost, r.moves, r.status, trace


_LIB.impl("three_opt_descent", _three_opt_descent, "CUDA")


def _guided_or_opt(tour, cost, D, guides, outer_iters, iter0, k, penalty, perturbation_moves, max_seg, reverse, max_moves, max_steps,
                   trace_capacity):
    r = ops.guided_or_opt_launch(tour, cost, D, guides, outer_iters, k, None if penalty is None else penalty.clone().contiguous(),
                                 perturbation_moves, max_seg, reverse, max_moves if max_moves > 0 else None,
                                 max_steps if max_steps > 0 else None, iter0, trace_capacity)
    trace = r.trace_cost if r.trace_cost is not None else torch.zeros((tour.shape[0], 0), dtype=torch.float64, device=tour.device)
    return r.tour, r.cost, r.best_tour, r.best_cost, r.moves, r.steps, r.status, r.penalty, trace, r.trace_len


_LIB.impl("guided_or_opt", _guided_or_opt, "CUDA")


def _aco(D, H, ants, iters, iter0, rho, min_ratio, gb_every, spread_starts, seed, u, tau, best_tour, best_cost):
    r = ops.aco_launch(D, H, ants, iters, rho, min_ratio if min_ratio > 0 else None, gb_every, spread_starts, seed, u, iter0,
                       None if tau is None else tau.clone().contiguous(), best_tour, best_cost, want_trace=True, want_ants=True)
    return r.best_tour, r.best_cost, r.tau, r.iters_done, r.status, r.trace_cost, r.ant_tours, r.ant_cost


_LIB.impl("aco", _aco, "CUDA")


def _beam_search(S, D, width, depot, select):
    r = ops.beam_search_launch(S, width, depot, D, select, want_beams=True)
    return r.best_tour, r.best_score, r.best_cost, r.n_beams, r.status, r.beam_tours, r.beam_score, r.beam_cost


_LIB.impl("beam_search", _beam_search, "CUDA")


def _greedy_edge(S, D, depot):
    r = ops.greedy_edge_launch(S, depot, D, want_edges=True)
    return r.tour, r.score, r.cost, r.edges, r.rounds, r.status


_LIB.impl("greedy_edge", _greedy_edge, "CUDA")


# ---- shape functions (fake tensors / tracing); no arithmetic -------------------------------------------------------
@torch.library.register_fake("gnngls::regret_forward")
def _(feat, packed_weights, n, heads, head_dim, hidden, layers):
    N = n * (n - 1) // 2
    in_dim = 1 if feat.dim() == 2 else feat.shape[-1]
    return feat.new_empty((feat.numel() // (N * in_dim), N), dtype=torch.float32)


def _table_shape(tour, D):
    B, n1 = tour.shape
    return D.new_empty((B, n1, n1), dtype=torch.float64)


torch.library.register_fake("gnngls::two_opt_delta_all")(_table_shape)
torch.library.register_fake("gnngls::relocate_delta_all")(_table_shape)


@torch.library.register_fake("gnngls::local_search")
def _(tour, cost, D, first_improvement):
    return torch.empty_like(tour), torch.empty_like(cost), tour.new_empty((tour.shape[0],), dtype=torch.int32)


@torch.library.register_fake("gnngls::gls_run")
def _(D, guides, init_tour, init_cost, perturbation_moves, max_outer_iters, time_limit_s, first_improvement, trace_capacity):
    B = D.shape[0]
    return (torch.empty_like(init_tour), torch.empty_like(init_cost), D.new_empty((B,), dtype=torch.int64),
            D.new_empty((B, trace_capacity), dtype=torch.float64), D.new_empty((B,), dtype=torch.int32))


@torch.library.register_fake("gnngls::insertion")
def _(W, depot, mode, order):
    return W.new_empty((W.shape[0], W.shape[1] + 1), dtype=torch.int32)


@torch.library.register_fake("gnngls::cheapest_insertion")
def _(sub_tour, node, W):
    return sub_tour.new_empty((sub_tour.shape[0], sub_tour.shape[1] + 1)), W.new_empty((W.shape[0],), dtype=torch.float64)


@torch.library.register_fake("gnngls::one_tree_bound")
def _(D, ub, max_iters):
    B, n = D.shape[0], D.shape[1]
    i32 = lambda: D.new_empty((B,), dtype=torch.int32)  # noqa: E731
    return D.new_empty((B,), dtype=torch.float64), D.new_empty((B, n), dtype=torch.float64), i32(), i32(), i32()


@torch.library.register_fake("gnngls::alpha_nearness")
def _(D, pi):
    return D.new_empty(tuple(D.shape), dtype=torch.float64)


@torch.library.register_fake("gnngls::or_opt_descent")
def _(tour, cost, D, max_seg, reverse, max_moves, trace_cap):
    B = tour.shape[0]
    i32 = lambda: tour.new_empty((B,), dtype=torch.int32)  # noqa: E731
    return (tour.new_empty(tuple(tour.shape)), cost.new_empty((B,)), i32(), i32(),
            cost.new_empty((B, max(int(trace_cap), 0)), dtype=torch.float64))


@torch.library.register_fake("gnngls::sample_nn_tours")
def _(W, R, depot, invert, seed, u):
    B, n = W.shape[0], W.shape[1]
    return W.new_empty((B, R, n + 1), dtype=torch.int32), W.new_empty((B, R), dtype=torch.int32)


@torch.library.register_fake("gnngls::ils")
def _(tour, cost, D, kicks, kick0, max_seg, reverse, max_moves, seed, u):
    B = tour.shape[0]
    i32 = lambda: tour.new_empty((B,), dtype=torch.int32)  # noqa: E731
    return (tour.new_empty(tuple(tour.shape)), cost.new_empty((B,)), i32(), i32(), i32(),
            cost.new_empty((B, max(int(kicks), 0)), dtype=torch.float64))


@torch.library.register_fake("gnngls::three_opt_descent")
def _(tour, cost, D, max_moves, trace_capacity):
    B = tour.shape[0]
    i32 = lambda: tour.new_empty((B,), dtype=torch.int32)  # noqa: E731
    return (tour.new_empty(tuple(tour.shape)), cost.new_empty((B,)), i32(), i32(),
            cost.new_empty((B, max(int(trace_capacity), 0)), dtype=torch.float64))


@torch.library.register_fake("gnngls::guided_or_opt")
def _(tour, cost, D, guides, outer_iters, iter0, k, penalty, perturbation_moves, max_seg, reverse, max_moves, max_steps, trace_capacity):
    B, n = tour.shape[0], D.shape[1]
    i32 = lambda: tour.new_empty((B,), dtype=torch.int32)  # noqa: E731
    return (tour.new_empty(tuple(tour.shape)), cost.new_empty((B,)), tour.new_empty(tuple(tour.shape)), cost.new_empty((B,)), i32(), i32(),
            i32(), tour.new_empty((B, n, n), dtype=torch.int32), cost.new_empty((B, max(int(trace_capacity), 0)), dtype=torch.float64),
            i32())


@torch.library.register_fake("gnngls::aco")
def _(D, H, ants, iters, iter0, rho, min_ratio, gb_every, spread_starts, seed, u, tau, best_tour, best_cost):
    B, n = D.shape[0], D.shape[1]
    i32 = lambda: D.new_empty((B,), dtype=torch.int32)  # noqa: E731
    return (D.new_empty((B, n + 1), dtype=torch.int32), D.new_empty((B,), dtype=torch.float64), D.new_empty((B, n, n), dtype=torch.float64),
            i32(), i32(), D.new_empty((B, max(int(iters), 0)), dtype=torch.float64),
            D.new_empty((B, max(int(ants), 0), n + 1), dtype=torch.int32), D.new_empty((B, max(int(ants), 0)), dtype=torch.float64))


@torch.library.register_fake("gnngls::beam_search")
def _(S, D, width, depot, select):
    B, n, W = S.shape[0], S.shape[1], max(int(width), 0)
    i32 = lambda: S.new_empty((B,), dtype=torch.int32)  # noqa: E731
    f64 = lambda: S.new_empty((B,), dtype=torch.float64)  # noqa: E731
    return (S.new_empty((B, n + 1), dtype=torch.int32), f64(), f64(), i32(), i32(), S.new_empty((B, W, n + 1), dtype=torch.int32),
            S.new_empty((B, W), dtype=torch.float64), S.new_empty((B, W), dtype=torch.float64))


@torch.library.register_fake("gnngls::greedy_edge")
def _(S, D, depot):
    B, n = S.shape[0], S.shape[1]
    i32 = lambda: S.new_empty((B,), dtype=torch.int32)  # noqa: E731
    f64 = lambda: S.new_empty((B,), dtype=torch.float64)  # noqa: E731
    return S.new_empty((B, n + 1), dtype=torch.int32), f64(), f64(), S.new_empty((B, n, 2), dtype=torch.int32), i32(), i32()
