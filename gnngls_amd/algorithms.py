"""Mirror of gnngls/algorithms.py (reference algorithms.py:9-195): `nearest_neighbor`, `cheapest_insertion`,
`insertion`, `local_search`, `guided_local_search` with the reference's signatures, return values and side
effects, executed by the HIP kernels (the persistent search kernel, the one-launch insertion constructor).
`alpha_nearness` (no counterpart in the reference) writes a model-free guide attribute for guided_local_search;
`beam_search` (no counterpart either) decodes a tour from an edge attribute by beam search, `greedy_edge` by greedy edge matching;
`or_opt_descent` (no counterpart either) is local_search with Or-opt in relocate's place, `iterated_local_search` is that
descent inside a loop of double-bridge kicks, and `three_opt_descent` is local_search with the exhaustive 3-opt scan in relocate's
place.

The probabilistic constructors (algorithms.py:21-64: `probabilistic_nearest_neighbour`, `best_probabilistic_nearest_neighbour`)
have the reference's signatures plus a trailing `seed` and the reference's LAW, not its draws: np.random.choice draws from NumPy's
stream against a pairwise `np.sum(p)`, the sampling kernel draws from Philox4x32-10 against the fixed summation order
include/gnngls_hip.h states.  Given the uniforms a walk is pinned bit for bit (ops.sample_nn_tours(u=...)); the distribution
over tours is the reference's (tests/golden/pnn_law_n6.npz).  seed=None takes the seed as ONE draw from NumPy's global stream,
so np.random.seed(k) makes a run repeatable as it does in the reference (the stream advances by one draw, not by n - 1).
"""
import time
import warnings

import networkx as nx
import numpy as np
import torch

from . import ops

TRACE_CAP = 1 << 16          # per-move trace entries that are always available
TRACE_PER_SECOND = 500_000   # extra entries per second of budget (a TSP100 search accepts ~2e5 moves per second)
TRACE_CAP_MAX = 1 << 25      # 400 MB of device memory for one instance's trace: beyond this the record degrades (see _progress)
IMP_CAP = 4096


class SearchAborted(RuntimeWarning):
    """The device watchdog stopped a search early: the returned tour is the best found so far."""


def _trace_cap(budget_s):
    return int(min(TRACE_CAP + TRACE_PER_SECOND * max(budget_s, 0.0), TRACE_CAP_MAX))


def _attr_matrix(G, attr):
    """nx.attr_matrix(G, attr)[0] for nodes 0..n-1 (algorithms.py:140,163): symmetric n x n fp64."""
    n = len(G.nodes)
    M = np.zeros((n, n), dtype=np.float64)
    for u, v, w in G.edges(data=attr):
        M[u, v] = w
        M[v, u] = w
    return M


def nearest_neighbor(G, depot, weight="weight"):
    """algorithms.py:9-18 (greedy on G.edges[(i,j)][weight]; ties -> first neighbour = lowest id)."""
    W = ops.as_dev(_attr_matrix(G, weight)[None], torch.float64)
    return ops.nearest_neighbor(W, depot)[0].tolist()


def cheapest_insertion(G, sub_tour, n, weight="weight"):
    """algorithms.py:67-79: `n` is the node to insert; the first position with the strictly smallest tour_cost wins.
    A sub-tour of fewer than two entries has no position (the reference's loop is empty): None."""
    if len(sub_tour) < 2:
        return None
    W = ops.as_dev(_attr_matrix(G, weight)[None], torch.float64)
    tour, _ = ops.cheapest_insertion(ops.as_dev(np.asarray(sub_tour, dtype=np.int32)[None], torch.int32),
                                     ops.as_dev(np.asarray([n], dtype=np.int32), torch.int32), W)
    return tour[0].tolist()


def insertion(G, depot, mode="farthest", weight="weight"):
    """algorithms.py:82-108.  mode 'random' draws its nodes with the reference's np.random.choice calls on the host
    (ops.random_order), so NumPy's global stream ends where the reference leaves it."""
    assert mode in ['random', 'nearest', 'farthest'], f'Unknown mode: {mode}'
    W = ops.as_dev(_attr_matrix(G, weight)[None], torch.float64)
    return ops.insertion(W, depot, mode)[0].tolist()


def _draw_seed(seed):
    return int(np.random.randint(0, 2 ** 63 - 1, dtype=np.int64)) if seed is None else int(seed)


def probabilistic_nearest_neighbour(G, depot, guide='weight', invert=True, seed=None):
    """algorithms.py:21-50: a nearest-neighbour walk whose next node is drawn with probability proportional to the guide (invert:
    to its reciprocal) among the unvisited ones.  Weights np.random.choice refuses raise ValueError as there."""
    n = len(G.nodes)
    seed = _draw_seed(seed)
    if n < 3:                                                                    # nothing to draw: one candidate per step
        return [depot] + [j for j in range(n) if j != depot] + [depot]
    W = ops.as_dev(_attr_matrix(G, guide)[None], torch.float64)
    return ops.sample_nn_tours(W, 1, depot, invert, seed)[0][0, 0].tolist()


def best_probabilistic_nearest_neighbour(G, depot, n_iters, guide='weight', weight='weight', seed=None):
    """algorithms.py:53-64: the first strictly cheapest (tour_cost on `weight`) of n_iters walks on `guide`, inverted as the
    reference's call leaves it; None for n_iters <= 0.  The walks are runs 0 .. n_iters-1 of one launch under `seed`."""
    n = len(G.nodes)
    seed = _draw_seed(seed)
    if n_iters <= 0:
        return None
    if n < 3:
        return [depot] + [j for j in range(n) if j != depot] + [depot]
    W = ops.as_dev(_attr_matrix(G, guide)[None], torch.float64)
    D = W if weight == guide else ops.as_dev(_attr_matrix(G, weight)[None], torch.float64)
    return ops.best_sampled_tour(W, D, int(n_iters), depot, True, seed)[0][0].tolist()


def alpha_nearness(G, weight="weight", attr="alpha", max_iters=2000):
    """Writes Helsgaun's alpha-nearness of every edge of G as the edge attribute `attr` (the reference has no counterpart; it is
    the classical relaxation of the regret its model predicts) and returns G: guided_local_search(G, ..., guides=["alpha"]) then
    runs as it does on any other guide.  The potentials come from the Held-Karp ascent of ops.one_tree_bound on `weight` with at
    most `max_iters` 1-trees and ub = the nearest-neighbour tour's length (max_iters=0: zero potentials)."""
    D = ops.as_dev(_attr_matrix(G, weight)[None], torch.float64)
    pi = None
    if max_iters > 0:
        pi = ops.one_tree_bound(D, ops.tour_cost(ops.nearest_neighbor(D), D), max_iters=int(max_iters)).pi
    A = ops.alpha_nearness(D, pi)[0].cpu().numpy()
    nx.set_edge_attributes(G, {(u, v): float(A[u, v]) for u, v in G.edges}, attr)
    return G


def beam_search(G, depot, width, guide='regret_pred', weight='weight', select='cost'):
    """A tour of G decoded from the edge attribute `guide` (smaller = better: a regret prediction, alpha, a distance, -log p) by beam
    search of `width` paths from `depot` on the GPU (ops.beam_search; no counterpart in the reference, whose paper compares against
    this decoder).  select 'cost': the shortest of the final beams on `weight`; 'score': the beam of the least summed guide.
    width = 1 is the greedy decode, nearest_neighbor(G, depot, weight=guide) where the partial sums are exact."""
    S = ops.as_dev(_attr_matrix(G, guide)[None], torch.float64)
    D = S if weight == guide else ops.as_dev(_attr_matrix(G, weight)[None], torch.float64)
    return ops.beam_search(S, int(width), depot, D, select).best_tour[0].tolist()


def greedy_edge(G, depot=0, guide='regret_pred', weight='weight'):
    """A tour of G decoded from the edge attribute `guide` (smaller = better: a regret prediction, alpha, a distance, -log p) by greedy
    edge matching on the GPU (ops.greedy_edge; no counterpart in the reference): the edges in ascending (guide, i, j), each accepted
    if both ends have degree below 2 and it closes no subtour, the path closed at the end.  The tour starts and ends at `depot` and
    leaves it towards the smaller-numbered neighbour.  `weight` only names the lengths the result's cost is summed on."""
    S = ops.as_dev(_attr_matrix(G, guide)[None], torch.float64)
    D = S if weight == guide else ops.as_dev(_attr_matrix(G, weight)[None], torch.float64)
    return ops.greedy_edge(S, depot, D).tour[0].tolist()


def _check_status(r, what):
    st = r.status.cpu().numpy()
    if (st == ops.STATUS_WATCHDOG).any():
        warnings.warn(f"{what}: the device watchdog stopped {int((st == ops.STATUS_WATCHDOG).sum())} search(es) early; "
                      "the result is the best tour found so far (pass a larger watchdog_s)", SearchAborted, stacklevel=3)


def _progress(r, t_host):
    """search_progress of the reference: one {'time','cost'} per accepted move (algorithms.py:127-130,180-183).
    If more moves were accepted than the device trace holds, the tail is the bounded improvement record (the returned
    best whenever it improved) and a warning says so -- the list never silently stops short of the returned cost."""
    L, cap = int(r.trace_len[0]), r.trace_cost.shape[1]
    kept = min(L, cap)
    costs = r.trace_cost[0, :kept].tolist()
    times = r.trace_time[0, :kept].tolist()
    rows = [{"time": t_host + dt, "cost": c} for dt, c in zip(times, costs)]
    if L > cap:
        warnings.warn(f"search trace truncated: {L} accepted moves, {cap} kept; later entries are new-best events only",
                      RuntimeWarning, stacklevel=3)
        k = min(int(r.imp_len[0]), r.imp_cost.shape[1])
        t_cut = times[-1] if times else -1.0
        rows += [{"time": t_host + dt, "cost": c}
                 for dt, c in zip(r.imp_time[0, :k].tolist(), r.imp_cost[0, :k].tolist()) if dt > t_cut]
    return rows


def local_search(init_tour, init_cost, D, first_improvement=False):
    """algorithms.py:111-132 -> (cur_tour, cur_cost, search_progress)."""
    D = np.asarray(D, dtype=np.float64)
    if not np.array_equal(D, D.T):
        # two_opt_cost assumes D[x,y] == D[y,x] (a reversal flips every inner edge), so on an asymmetric matrix the
        # reference's descent is not a descent at all and need not terminate; refuse instead of spinning
        raise NotImplementedError("local_search needs a symmetric distance matrix "
                                  "(nx.attr_matrix of an undirected graph always is)")
    t0 = time.time()
    r = ops.gls_run(ops.as_dev(D[None], torch.float64), None,
                    ops.as_dev(np.asarray(init_tour, dtype=np.int32)[None], torch.int32),
                    ops.as_dev(np.asarray([init_cost], dtype=np.float64), torch.float64),
                    first_improvement=first_improvement, max_outer_iters=0, trace_cap=TRACE_CAP, want_trace_time=True,
                    imp_cap=IMP_CAP)
    _check_status(r, "local_search")
    return r.best_tour[0].tolist(), r.best_cost[0].item(), _progress(r, t0)


def or_opt_descent(init_tour, init_cost, D, max_seg=3, reverse=True):
    """local_search above with relocate_a2a replaced by the Or-opt scan (operators.or_opt_a2a: chains of 1..max_seg nodes,
    reversed too if `reverse`), best improvement, on the GPU (ops.or_opt_descent; no counterpart in the reference)
    -> (tour, cost, n_moves).  With max_seg=1, reverse=False it returns local_search's tour and cost."""
    r = ops.or_opt_descent(ops.as_dev(np.asarray(init_tour, dtype=np.int32)[None], torch.int32),
                           ops.as_dev(np.asarray([init_cost], dtype=np.float64), torch.float64),
                           ops.as_dev(np.asarray(D, dtype=np.float64)[None], torch.float64), max_seg, reverse)
    return r.tour[0].tolist(), r.cost[0].item(), int(r.moves[0])


def three_opt_descent(init_tour, init_cost, D):
    """local_search above with relocate_a2a replaced by the exhaustive 3-opt scan (operators.three_opt_a2a), best improvement, on
    the GPU (ops.three_opt_descent; no counterpart in the reference) -> (tour, cost, search_progress): one {'time', 'cost'} per
    applied move as local_search records them, every 'time' the moment the launch returned (the kernel keeps no clock)."""
    n = len(init_tour) - 1
    r = ops.three_opt_descent(ops.as_dev(np.asarray(init_tour, dtype=np.int32)[None], torch.int32),
                              ops.as_dev(np.asarray([init_cost], dtype=np.float64), torch.float64),
                              ops.as_dev(np.asarray(D, dtype=np.float64)[None], torch.float64), trace_cap=100 * n)
    moves = int(r.moves[0])
    t = time.time()
    return r.tour[0].tolist(), r.cost[0].item(), [{"time": t, "cost": c} for c in r.trace_cost[0, :moves].tolist()]


def iterated_local_search(init_tour, init_cost, D, kicks, max_seg=3, reverse=True, seed=None):
    """Iterated local search on the GPU (ops.ils; no counterpart in the reference): or_opt_descent above, then `kicks` times a
    double-bridge kick of the accepted tour, the same descent, and the better tour kept -> (tour, cost, costs_per_kick), the last
    the cost the descent reached after each kick.  seed=None takes the seed as ONE draw from NumPy's global stream."""
    seed = _draw_seed(seed)
    r = ops.ils(ops.as_dev(np.asarray(init_tour, dtype=np.int32)[None], torch.int32),
                ops.as_dev(np.asarray([init_cost], dtype=np.float64), torch.float64),
                ops.as_dev(np.asarray(D, dtype=np.float64)[None], torch.float64), int(kicks), max_seg, reverse, seed=seed,
                want_trace=True)
    return r.tour[0].tolist(), r.cost[0].item(), r.trace_cost[0].tolist()


def guided_local_search(G, init_tour, init_cost, t_lim, weight="weight", guides=["weight"], perturbation_moves=30,
                        first_improvement=False, max_outer_iters=None, watchdog_s=None):
    """algorithms.py:135-195 -> (best_tour, best_cost, search_progress).

    `t_lim` is an absolute time.time() deadline as in the reference.  Like the reference this
    writes the final 'penalty' edge attribute into G (algorithms.py:138,161).  `max_outer_iters`
    (extension) runs an exact number of outer iterations instead of the wall-clock budget; `watchdog_s` (extension)
    bounds the device time of the run (default: budget + 5 s, or a bound scaled to the requested iterations) -- a run
    stopped by it returns the best tour so far and raises a SearchAborted warning."""
    D = _attr_matrix(G, weight)                                                  # algorithms.py:140
    gm = np.stack([_attr_matrix(G, g) for g in guides])[:, None]                 # [G,1,n,n]
    t0 = time.time()
    remaining = max(t_lim - t0, 0.0)
    r = ops.gls_run(ops.as_dev(D[None], torch.float64), ops.as_dev(gm, torch.float64),
                    ops.as_dev(np.asarray(init_tour, dtype=np.int32)[None], torch.int32),
                    ops.as_dev(np.asarray([init_cost], dtype=np.float64), torch.float64),
                    perturbation_moves=perturbation_moves, first_improvement=first_improvement,
                    max_outer_iters=-1 if max_outer_iters is None else int(max_outer_iters), time_limit_s=remaining,
                    watchdog_s=watchdog_s, trace_cap=_trace_cap(remaining if max_outer_iters is None else 0.0),
                    want_trace_time=True, want_penalty=True, imp_cap=IMP_CAP)
    _check_status(r, "guided_local_search")
    pen = r.penalty[0].cpu().numpy()
    nx.set_edge_attributes(G, {(u, v): float(pen[u, v]) for u, v in G.edges}, "penalty")
    return r.best_tour[0].tolist(), r.best_cost[0].item(), _progress(r, t0)
