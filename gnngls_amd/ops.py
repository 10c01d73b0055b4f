"""Batched device API over the C ABI (include/gnngls_hip.h).

All tensors are torch CUDA tensors used as plain device buffers; every function enqueues HIP
kernels on the current torch stream through libgnngls_hip.so.  B = instances, n = nodes.
The reference-signature mirrors (operators.py / algorithms.py of this package) are thin
list-in/list-out wrappers over these.
"""
import ctypes
from dataclasses import dataclass

import torch

from . import _lib

OP_TWO_OPT = 0
OP_RELOCATE = 1


def _dev():
    if not torch.cuda.is_available():
        raise _lib.GnnglsHipError("no HIP device visible: gnngls_amd has no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


def as_dev(x, dtype):
    t = torch.as_tensor(x, dtype=dtype)
    return t.to(_dev()).contiguous()


def _check_shapes(tour, D):
    B, n1 = tour.shape
    n = n1 - 1
    assert D.shape == (B, n, n), f"D shape {tuple(D.shape)} does not match tours [{B},{n1}]"
    assert tour.dtype == torch.int32 and D.dtype == torch.float64
    return B, n


def two_opt_delta_all(tour, D):
    """[B,n+1,n+1] fp64 table of two_opt_cost (reference operators.py:14-29)."""
    B, n = _check_shapes(tour, D)
    out = torch.empty((B, n + 1, n + 1), dtype=torch.float64, device=tour.device)
    L = _lib.load()
    _lib.check(L.gnngls_two_opt_delta_all(_lib.ptr(tour), _lib.ptr(D), B, n, _lib.ptr(out), _lib.current_stream()),
               "two_opt_delta_all")
    return out


def relocate_delta_all(tour, D):
    """[B,n+1,n+1] fp64 table of relocate_cost (reference operators.py:83-103)."""
    B, n = _check_shapes(tour, D)
    out = torch.empty((B, n + 1, n + 1), dtype=torch.float64, device=tour.device)
    L = _lib.load()
    _lib.check(L.gnngls_relocate_delta_all(_lib.ptr(tour), _lib.ptr(D), B, n, _lib.ptr(out), _lib.current_stream()),
               "relocate_delta_all")
    return out


def best_move(tour, D, op, pos_i=None, first_improvement=False):
    """One a2a (pos_i None) or o2a scan.  Returns (delta[B], move[B,2], new_tour[B,n+1])."""
    B, n = _check_shapes(tour, D)
    delta = torch.empty((B,), dtype=torch.float64, device=tour.device)
    move = torch.empty((B, 2), dtype=torch.int32, device=tour.device)
    new_tour = torch.empty_like(tour)
    if pos_i is not None:
        assert pos_i.dtype == torch.int32 and pos_i.shape == (B,)
    L = _lib.load()
    _lib.check(L.gnngls_best_move(_lib.ptr(tour), _lib.ptr(D), B, n, int(op), _lib.ptr(pos_i), int(first_improvement),
                                  _lib.ptr(delta), _lib.ptr(move), _lib.ptr(new_tour), _lib.current_stream()),
               "best_move")
    return delta, move, new_tour


def tour_cost(tour, D):
    B, n = _check_shapes(tour, D)
    out = torch.empty((B,), dtype=torch.float64, device=tour.device)
    L = _lib.load()
    _lib.check(L.gnngls_tour_cost(_lib.ptr(tour), _lib.ptr(D), B, n, _lib.ptr(out), _lib.current_stream()), "tour_cost")
    return out


def nearest_neighbor(W, depot=0):
    """W [B,n,n] fp64 -> tours [B,n+1] int32 (reference algorithms.py:9-18)."""
    B, n, n2 = W.shape
    assert n == n2 and W.dtype == torch.float64
    out = torch.empty((B, n + 1), dtype=torch.int32, device=W.device)
    L = _lib.load()
    _lib.check(L.gnngls_nearest_neighbor(_lib.ptr(W), B, n, int(depot), _lib.ptr(out), _lib.current_stream()),
               "nearest_neighbor")
    return out


INSERT_MODES = {"nearest": 0, "farthest": 1, "random": 2}    # GNNGLS_INSERT_* (mode 'random' = GNNGLS_INSERT_GIVEN_ORDER)
INSERTION_MAX_N = 2048                                        # GNNGLS_INSERTION_MAX_N
STATUS_BAD_ORDER = 5


def random_order(n, depot=0):
    """The node order of insertion(G, depot, mode='random') (reference algorithms.py:85-91,105): np.random.choice on the
    shrinking list of outside nodes.  The draws do not depend on the tour, so they are made here with the very same calls:
    the same nodes, and NumPy's global stream is left where the reference leaves it."""
    import numpy as np
    nodes = list(range(n))
    nodes.remove(depot)
    order = []
    while len(nodes) > 0:
        next_node = np.random.choice(nodes)
        nodes.remove(next_node)
        order.append(int(next_node))
    return order


def insertion(W, depot=0, mode="farthest", order=None):
    """W [B,n,n] fp64 -> tours [B,n+1] int32 (reference algorithms.py:82-108), one launch for the whole batch.
    mode 'nearest' / 'farthest': algorithms.py:93-103.  mode 'random': `order` [B,n-1] int32 gives every instance's node
    order; None draws it per instance with random_order (the reference's np.random.choice calls, in batch order).
    A row of `order` that is not a permutation of the non-depot nodes raises."""
    assert mode in INSERT_MODES, f"Unknown mode: {mode}"
    B, n, n2 = W.shape
    assert n == n2 and W.dtype == torch.float64
    out = torch.empty((B, n + 1), dtype=torch.int32, device=W.device)
    status = None
    if mode == "random":
        if order is None:
            order = torch.tensor([random_order(n, int(depot)) for _ in range(B)], dtype=torch.int32).reshape(B, n - 1)
        order = order.to(device=W.device, dtype=torch.int32).contiguous()
        assert order.shape == (B, n - 1), f"order shape {tuple(order.shape)} is not [{B},{n - 1}]"
        status = torch.zeros((B,), dtype=torch.int32, device=W.device)
    else:
        assert order is None, "order is only read in mode 'random'"
    L = _lib.load()
    _lib.check(L.gnngls_insertion(_lib.ptr(W), B, n, int(depot), INSERT_MODES[mode], _lib.ptr(order) if n > 1 else None,
                                  _lib.ptr(out), _lib.ptr(status), _lib.current_stream()), "insertion")
    if status is not None:
        bad = status.nonzero().flatten().tolist()
        if bad:
            raise ValueError(f"insertion: order rows {bad[:8]} are not permutations of the non-depot nodes "
                             f"(status {STATUS_BAD_ORDER})")
    return out


def cheapest_insertion(sub_tour, node, W):
    """sub_tour [B,len] int32, node [B] int32, W [B,n,n] fp64 -> (tours [B,len+1] int32, cost [B] fp64): the first position whose
    candidate tour has the strictly smallest tour_cost (reference algorithms.py:67-79), and that cost."""
    B, n, n2 = W.shape
    assert n == n2 and W.dtype == torch.float64
    assert sub_tour.dtype == torch.int32 and sub_tour.dim() == 2 and sub_tour.shape[0] == B
    assert node.dtype == torch.int32 and node.shape == (B,)
    ln = sub_tour.shape[1]
    out = torch.empty((B, ln + 1), dtype=torch.int32, device=W.device)
    cost = torch.zeros((B,), dtype=torch.float64, device=W.device)
    L = _lib.load()
    _lib.check(L.gnngls_cheapest_insertion(_lib.ptr(sub_tour), ln, _lib.ptr(node), _lib.ptr(W), B, n, _lib.ptr(out), _lib.ptr(cost),
                                           _lib.current_stream()), "cheapest_insertion")
    if bool(torch.isnan(cost).any()):
        raise ValueError("cheapest_insertion: a sub-tour or node index is out of 0..n-1 (or a weight is NaN)")
    return out, cost


SAMPLE_MAX_N = 1024                                           # GNNGLS_SAMPLE_MAX_N
SAMPLE_BAD_WEIGHTS = 6                                        # GNNGLS_SAMPLE_BAD_WEIGHTS


def sample_nn_launch(W, R, depot=0, invert=True, seed=0, u=None):
    """The launch behind sample_nn_tours and torch.ops.gnngls.sample_nn_tours: -> (tours [B,R,n+1] int32, status [B,R] int32),
    nothing raised for a walk that met bad weights (its status is SAMPLE_BAD_WEIGHTS, its tour -1)."""
    B, n, n2 = W.shape
    assert n == n2 and W.dtype == torch.float64
    R = int(R)
    if u is not None:
        u = u.to(device=W.device, dtype=torch.float64).contiguous()
        assert u.shape == (B, R, n - 1), f"u shape {tuple(u.shape)} is not [{B},{R},{n - 1}]"
    tours = torch.empty((B, max(R, 0), n + 1), dtype=torch.int32, device=W.device)
    status = torch.zeros((B, max(R, 0)), dtype=torch.int32, device=W.device)
    L = _lib.load()
    if not hasattr(L, "gnngls_sample_nn_tours"):
        raise _lib.GnnglsHipError("this build of libgnngls_hip.so has no gnngls_sample_nn_tours")
    _lib.check(L.gnngls_sample_nn_tours(_lib.ptr(W.contiguous()), B, n, R, int(depot), int(bool(invert)),
                                        ctypes.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), _lib.ptr(u), _lib.ptr(tours), _lib.ptr(status),
                                        _lib.current_stream()), "sample_nn_tours")
    return tours, status


def sample_nn_tours(W, R, depot=0, invert=True, seed=0, u=None):
    """R sampled nearest-neighbour walks per instance (reference algorithms.py:21-50, probabilistic_nearest_neighbour), one
    launch, one wavefront per walk: W [B,n,n] fp64 -> (tours [B,R,n+1] int32, status [B,R] int32).  The next node is drawn with
    probability proportional to W[i,j] (invert: to 1 / W[i,j]) among the unvisited ones; include/gnngls_hip.h states the walk
    and the order of its sums.  u [B,R,n-1] fp64 in [0,1) gives the uniforms (the walks are then pinned bit for bit); None draws
    them on the device from Philox4x32-10 keyed by `seed` with counter (b, r, step) -- not NumPy's stream: against the
    reference the walks agree in law.  Weights np.random.choice would refuse (a zero under invert, NaN, negative) raise."""
    tours, status = sample_nn_launch(W, R, depot, invert, seed, u)
    bad = (status != 0).nonzero()
    if bad.shape[0]:
        raise ValueError(f"sample_nn_tours: walks (instance, run) {bad[:8].tolist()} met weights that are no probabilities "
                         f"(NaN, negative, infinite or zero under invert; status {SAMPLE_BAD_WEIGHTS}): probabilities do not sum to 1")
    return tours, status


def first_argmin(x):
    """[B,R] -> [B] int64 index of the first strictly smallest entry of every row."""
    R = x.shape[1]
    idx = torch.arange(R, device=x.device).expand_as(x)
    return torch.where(x == x.min(dim=1, keepdim=True).values, idx, torch.full_like(idx, R)).min(dim=1).values


def best_sampled_tour(W, D, R, depot=0, invert=True, seed=0, u=None):
    """The first strictly cheapest of R sampled walks per instance under tour_cost on D (reference algorithms.py:53-64,
    best_probabilistic_nearest_neighbour): W, D [B,n,n] fp64 -> (tour [B,n+1] int32, cost [B] fp64)."""
    B, n, _ = W.shape
    assert D.shape == W.shape and D.dtype == torch.float64
    tours, _ = sample_nn_tours(W, R, depot, invert, seed, u)
    cost = torch.stack([tour_cost(tours[:, r].contiguous(), D) for r in range(tours.shape[1])], dim=1)      # [B,R]
    k = first_argmin(cost)
    rows = torch.arange(B, device=W.device)
    return tours[rows, k].contiguous(), cost[rows, k].contiguous()


@dataclass
class GlsResult:
    best_tour: torch.Tensor      # [B,n+1] int32
    best_cost: torch.Tensor      # [B] fp64
    outer_iters: torch.Tensor    # [B] int64
    trace_cost: torch.Tensor     # [B,T] fp64 or None
    trace_time: torch.Tensor     # [B,T] fp32 or None
    trace_len: torch.Tensor      # [B] int32
    penalty: torch.Tensor        # [B,n,n] int32 or None
    evals: torch.Tensor          # [B] int64
    status: torch.Tensor         # [B] int32
    imp_cost: torch.Tensor = None   # [B,imp_cap] fp64: the returned best after every improvement (algorithms.py:143,190-191)
    imp_time: torch.Tensor = None   # [B,imp_cap] fp32 seconds since the workgroup started
    imp_iter: torch.Tensor = None   # [B,imp_cap] int64 completed outer iterations at that moment
    imp_len: torch.Tensor = None    # [B] int32 number of improvements (may exceed imp_cap)

    @property
    def trace_truncated(self):
        """[B] bool: more moves were accepted than the per-move trace could hold."""
        cap = 0 if self.trace_cost is None else self.trace_cost.shape[1]
        return self.trace_len > cap


STATUS_OK, STATUS_WATCHDOG, STATUS_PENALTY_OVERFLOW, STATUS_ASYMMETRIC = 0, 1, 2, 3


ONE_TREE_MAX_N = 1024                                         # GNNGLS_ONE_TREE_MAX_N
BOUND_EXIT_ITERS, BOUND_EXIT_STEP, BOUND_EXIT_TOUR = 0, 1, 2  # GNNGLS_BOUND_EXIT_*


@dataclass
class OneTreeResult:
    bound: torch.Tensor          # [B] fp64: max_k w(pi_k) <= the optimal tour length
    pi: torch.Tensor             # [B,n] fp64 potentials that attain it, or None
    iters: torch.Tensor          # [B] int32 1-trees built
    exit_kind: torch.Tensor      # [B] int32 BOUND_EXIT_* (TOUR: the bound is the optimum)
    status: torch.Tensor         # [B] int32


def one_tree_bound(D, ub, max_iters=2000, want_pi=True):
    """Held-Karp 1-tree lower bounds of the optimal tour lengths of a batch, one launch (oracle/one_tree.c bit for bit; stands in
    for Concorde's optimum in the reference's gap, scripts/test.py:62,104).  D [B,n,n] fp64 bitwise symmetric, ub [B] fp64 the
    length of any tour per instance (steers the step size only).  A matrix that is not symmetric raises."""
    B, n, n2 = D.shape
    assert n == n2 and D.dtype == torch.float64
    assert ub.dtype == torch.float64 and ub.shape == (B,), f"ub shape {tuple(ub.shape)} is not [{B}]"
    dev = D.device
    bound = torch.empty((B,), dtype=torch.float64, device=dev)
    pi = torch.zeros((B, n), dtype=torch.float64, device=dev) if want_pi else None
    iters = torch.zeros((B,), dtype=torch.int32, device=dev)
    exit_kind = torch.zeros((B,), dtype=torch.int32, device=dev)
    status = torch.zeros((B,), dtype=torch.int32, device=dev)
    L = _lib.load()
    if not hasattr(L, "gnngls_one_tree_bound"):
        raise _lib.GnnglsHipError("this build of libgnngls_hip.so has no gnngls_one_tree_bound")
    _lib.check(L.gnngls_one_tree_bound(_lib.ptr(D.contiguous()), _lib.ptr(ub.contiguous()), B, n, int(max_iters), _lib.ptr(bound),
                                       _lib.ptr(pi), _lib.ptr(iters), _lib.ptr(exit_kind), _lib.ptr(status), _lib.current_stream()),
               "one_tree_bound")
    bad = (status == STATUS_ASYMMETRIC).nonzero().flatten().tolist()
    if bad:
        raise ValueError(f"one_tree_bound: the matrices of instances {bad[:8]} are not bitwise symmetric (status {STATUS_ASYMMETRIC}): "
                         "the 1-tree bound is a bound for symmetric costs only")
    return OneTreeResult(bound, pi, iters, exit_kind, status)


def one_tree_describe(n):
    """-> dict(threads, lds_bytes, nodes_per_lane, form) of the launch one_tree_bound makes for n nodes (host-side query)."""
    vals = [ctypes.c_int(0) for _ in range(3)]
    _lib.check(_lib.load().gnngls_one_tree_bound_describe(int(n), *[ctypes.cast(ctypes.byref(v), ctypes.c_void_p) for v in vals]),
               "one_tree_bound_describe")
    t, lds, slots = (v.value for v in vals)
    return {"threads": t, "lds_bytes": lds, "nodes_per_lane": slots,
            "form": f"{t // 64} wavefront(s) per instance, {slots} node(s) per lane in registers, matrix rows from global memory"}


ALPHA_MAX_N = 1024                                            # GNNGLS_ALPHA_MAX_N


def alpha_nearness(D, pi=None):
    """Helsgaun's alpha-nearness of every edge of a batch, one launch: alpha(e) = (minimum 1-tree forced through e) - (minimum
    1-tree) under the potentials pi (include/gnngls_hip.h states the definition; host.alpha_nearness restates it in NumPy, bit
    for bit).  D [B,n,n] fp64 bitwise symmetric, pi [B,n] fp64 (one_tree_bound(...).pi) or None (all zeros) -> alpha [B,n,n]
    fp64, symmetric, >= 0, +0.0 on the diagonal and on the edges of the minimum 1-tree: a guide matrix for gls_run.  A matrix
    that is not symmetric raises."""
    B, n, n2 = D.shape
    assert n == n2 and D.dtype == torch.float64
    if pi is not None:
        assert pi.dtype == torch.float64 and pi.shape == (B, n), f"pi shape {tuple(pi.shape)} is not [{B},{n}]"
        pi = pi.to(D.device).contiguous()
    out = torch.empty((B, n, n), dtype=torch.float64, device=D.device)
    status = torch.zeros((B,), dtype=torch.int32, device=D.device)
    L = _lib.load()
    if not hasattr(L, "gnngls_alpha_nearness"):
        raise _lib.GnnglsHipError("this build of libgnngls_hip.so has no gnngls_alpha_nearness")
    _lib.check(L.gnngls_alpha_nearness(_lib.ptr(D.contiguous()), _lib.ptr(pi), B, n, _lib.ptr(out), _lib.ptr(status),
                                       _lib.current_stream()), "alpha_nearness")
    bad = (status == STATUS_ASYMMETRIC).nonzero().flatten().tolist()
    if bad:
        raise ValueError(f"alpha_nearness: the matrices of instances {bad[:8]} are not bitwise symmetric (status {STATUS_ASYMMETRIC}): "
                         "alpha-nearness is defined for symmetric costs only")
    return out


OR_OPT_MAX_N = 1024                                           # GNNGLS_OR_OPT_MAX_N
OR_OPT_MAX_SEG = 3                                            # GNNGLS_OR_OPT_MAX_SEG
STATUS_MOVE_CAP = 6                                           # GNNGLS_STATUS_MOVE_CAP


@dataclass
class OrOptResult:
    tour: torch.Tensor           # [B,n+1] int32
    cost: torch.Tensor           # [B] fp64: the start cost plus the deltas of the applied moves, in order
    moves: torch.Tensor          # [B] int32 applied moves (2-opt and Or-opt)
    status: torch.Tensor         # [B] int32 STATUS_OK (a local optimum of both scans) or STATUS_MOVE_CAP
    trace_cost: torch.Tensor     # [B,trace_cap] fp64 the cost after each of the first trace_cap moves, or None


def _or_opt_entry(name):
    L = _lib.load()
    if not hasattr(L, name):
        raise _lib.GnnglsHipError(f"this build of libgnngls_hip.so has no {name}")
    return getattr(L, name)


def _raise_asymmetric(what, bad, why="the Or-opt kernels read D[d,s] as D[s][d]"):
    raise ValueError(f"{what}: the matrices of instances {bad[:8]} are not bitwise symmetric (status {STATUS_ASYMMETRIC}): {why}")


def or_opt_best_move(tour, D, max_seg=3, reverse=True):
    """One best-improvement scan of the Or-opt neighbourhood of every tour of a batch, one launch: a chain of 1..max_seg
    consecutive nodes moves between two other tour neighbours, forward or (reverse, chains of two and three) reversed
    (include/gnngls_hip.h states the candidates, the delta and the order; host.or_opt_a2a restates them in NumPy, bit for bit).
    tour [B,n+1] int32, D [B,n,n] fp64 bitwise symmetric -> (delta [B] fp64, 0.0 when nothing qualifies; move [B,4] int32 =
    i, L, rev, j, -1s when none; new_tour [B,n+1] int32).  A matrix that is not symmetric raises."""
    B, n = _check_shapes(tour, D)
    delta = torch.empty((B,), dtype=torch.float64, device=tour.device)
    move = torch.empty((B, 4), dtype=torch.int32, device=tour.device)
    new_tour = torch.empty_like(tour)
    f = _or_opt_entry("gnngls_or_opt_best_move")
    _lib.check(f(_lib.ptr(tour.contiguous()), _lib.ptr(D.contiguous()), B, n, int(max_seg), int(bool(reverse)), _lib.ptr(delta),
                 _lib.ptr(move), _lib.ptr(new_tour), _lib.current_stream()), "or_opt_best_move")
    bad = torch.isnan(delta).nonzero().flatten().tolist()
    if bad:
        _raise_asymmetric("or_opt_best_move", bad)
    return delta, move, new_tour


def or_opt_launch(tour, cost, D, max_seg=3, reverse=True, max_moves=None, trace_cap=0):
    """The launch behind or_opt_descent and torch.ops.gnngls.or_opt_descent: -> OrOptResult, nothing raised for an instance
    whose matrix is not symmetric (its status is STATUS_ASYMMETRIC, its outputs are its inputs)."""
    B, n = _check_shapes(tour, D)
    assert cost.dtype == torch.float64 and cost.shape == (B,), f"cost shape {tuple(cost.shape)} is not [{B}]"
    max_moves = 100 * n if max_moves is None else int(max_moves)
    trace_cap = int(trace_cap)
    dev = tour.device
    tour_out = torch.empty_like(tour)
    cost_out = torch.empty((B,), dtype=torch.float64, device=dev)
    moves = torch.zeros((B,), dtype=torch.int32, device=dev)
    status = torch.zeros((B,), dtype=torch.int32, device=dev)
    trace = torch.zeros((B, trace_cap), dtype=torch.float64, device=dev) if trace_cap > 0 else None
    f = _or_opt_entry("gnngls_or_opt_descent")
    _lib.check(f(_lib.ptr(tour.contiguous()), _lib.ptr(cost.contiguous()), _lib.ptr(D.contiguous()), B, n, int(max_seg),
                 int(bool(reverse)), max_moves, _lib.ptr(tour_out), _lib.ptr(cost_out), _lib.ptr(moves), _lib.ptr(status),
                 _lib.ptr(trace), trace_cap, _lib.current_stream()), "or_opt_descent")
    return OrOptResult(tour_out, cost_out, moves, status, trace)


def or_opt_descent(tour, cost, D, max_seg=3, reverse=True, max_moves=None, trace_cap=0):
    """The reference's local_search (algorithms.py:111-132) with relocate_a2a replaced by the Or-opt scan of or_opt_best_move:
    two_opt_a2a and the Or-opt scan alternate, best improvement, cost += delta after each move, until a full pass moves nothing
    (status STATUS_OK) or max_moves moves are applied (STATUS_MOVE_CAP; None = 100 * n).  One launch for the batch, bit for bit
    host.or_opt_descent; with max_seg=1, reverse=False it is local_search itself.  tour [B,n+1] int32, cost [B] fp64, D [B,n,n]
    fp64 bitwise symmetric -> OrOptResult.  A matrix that is not symmetric raises."""
    r = or_opt_launch(tour, cost, D, max_seg, reverse, max_moves, trace_cap)
    bad = (r.status == STATUS_ASYMMETRIC).nonzero().flatten().tolist()
    if bad:
        _raise_asymmetric("or_opt_descent", bad)
    return r


THREE_OPT_MAX_N = 256                                         # GNNGLS_THREE_OPT_MAX_N


@dataclass
class ThreeOptResult:
    tour: torch.Tensor           # [B,n+1] int32
    cost: torch.Tensor           # [B] fp64: the start cost plus the deltas of the applied moves, in order
    moves: torch.Tensor          # [B] int32 applied moves (2-opt and 3-opt)
    status: torch.Tensor         # [B] int32 STATUS_OK (a local optimum of both scans) or STATUS_MOVE_CAP
    trace_cost: torch.Tensor     # [B,trace_cap] fp64 the cost after each of the first trace_cap moves, or None


_THREE_OPT_READS = "the 3-opt kernels read D[c2,b1] as D[b1][c2]"


def three_opt_lds_max_n():
    """The largest n whose distance triangle the 3-opt kernels of this build stage in LDS; larger instances read D from global
    memory (the results are the same bit for bit)."""
    return int(_or_opt_entry("gnngls_three_opt_lds_max_n")())


def three_opt_best_move(tour, D):
    """One best-improvement scan of the 3-opt neighbourhood of every tour of a batch, one launch: the tour edges at positions
    p1 < p2 < p3 leave and the pieces between them are reconnected in the four ways that are no 2-opt move, all C(n,3) x 4
    candidates (include/gnngls_hip.h states the candidates, the delta and the order; host.three_opt_a2a restates them in NumPy, bit
    for bit).  tour [B,n+1] int32, D [B,n,n] fp64 bitwise symmetric, 3 <= n <= THREE_OPT_MAX_N -> (delta [B] fp64, 0.0 when nothing
    qualifies; move [B,4] int32 = p1, p2, p3, kind, -1s when none; new_tour [B,n+1] int32).  A matrix that is not symmetric
    raises."""
    B, n = _check_shapes(tour, D)
    delta = torch.empty((B,), dtype=torch.float64, device=tour.device)
    move = torch.empty((B, 4), dtype=torch.int32, device=tour.device)
    new_tour = torch.empty_like(tour)
    f = _or_opt_entry("gnngls_three_opt_best_move")
    _lib.check(f(_lib.ptr(tour.contiguous()), _lib.ptr(D.contiguous()), B, n, _lib.ptr(delta), _lib.ptr(move), _lib.ptr(new_tour),
                 _lib.current_stream()), "three_opt_best_move")
    bad = torch.isnan(delta).nonzero().flatten().tolist()
    if bad:
        _raise_asymmetric("three_opt_best_move", bad, _THREE_OPT_READS)
    return delta, move, new_tour


def three_opt_launch(tour, cost, D, max_moves=None, trace_cap=0):
    """The launch behind three_opt_descent and torch.ops.gnngls.three_opt_descent: -> ThreeOptResult, nothing raised for an
    instance whose matrix is not symmetric (its status is STATUS_ASYMMETRIC, its outputs are its inputs)."""
    B, n = _check_shapes(tour, D)
    assert cost.dtype == torch.float64 and cost.shape == (B,), f"cost shape {tuple(cost.shape)} is not [{B}]"
    max_moves = 100 * n if max_moves is None else int(max_moves)
    trace_cap = int(trace_cap)
    dev = tour.device
    tour_out = torch.empty_like(tour)
    cost_out = torch.empty((B,), dtype=torch.float64, device=dev)
    moves = torch.zeros((B,), dtype=torch.int32, device=dev)
    status = torch.zeros((B,), dtype=torch.int32, device=dev)
    trace = torch.zeros((B, trace_cap), dtype=torch.float64, device=dev) if trace_cap > 0 else None
    f = _or_opt_entry("gnngls_three_opt_descent")
    _lib.check(f(_lib.ptr(tour.contiguous()), _lib.ptr(cost.contiguous()), _lib.ptr(D.contiguous()), B, n, max_moves,
                 _lib.ptr(tour_out), _lib.ptr(cost_out), _lib.ptr(moves), _lib.ptr(status), _lib.ptr(trace), trace_cap,
                 _lib.current_stream()), "three_opt_descent")
    return ThreeOptResult(tour_out, cost_out, moves, status, trace)


def three_opt_descent(tour, cost, D, max_moves=None, trace_cap=0):
    """The reference's local_search (algorithms.py:111-132) with relocate_a2a replaced by the 3-opt scan of three_opt_best_move:
    two_opt_a2a and the 3-opt scan alternate, best improvement, cost += delta after each move, until a full pass moves nothing
    (status STATUS_OK) or max_moves moves are applied (STATUS_MOVE_CAP; None = 100 * n).  One launch for the batch, bit for bit
    host.three_opt_descent.  tour [B,n+1] int32, cost [B] fp64, D [B,n,n] fp64 bitwise symmetric, 3 <= n <= THREE_OPT_MAX_N
    -> ThreeOptResult.  A matrix that is not symmetric raises."""
    r = three_opt_launch(tour, cost, D, max_moves, trace_cap)
    bad = (r.status == STATUS_ASYMMETRIC).nonzero().flatten().tolist()
    if bad:
        _raise_asymmetric("three_opt_descent", bad, _THREE_OPT_READS)
    return r


@dataclass
class IlsResult:
    tour: torch.Tensor           # [B,n+1] int32 the accepted tour
    cost: torch.Tensor           # [B] fp64 its accumulated cost
    moves: torch.Tensor          # [B] int32 applied descent moves of the whole run, the first descent's included
    accepted: torch.Tensor       # [B] int32 accepted kicks
    status: torch.Tensor         # [B] int32 STATUS_OK, STATUS_MOVE_CAP or (ils_launch only) STATUS_ASYMMETRIC
    trace_cost: torch.Tensor     # [B,kicks] fp64 the candidate's cost after every kick (NaN: the kick never ran), or None


def ils_launch(tour, cost, D, kicks, max_seg=3, reverse=True, max_moves=None, seed=0, u=None, kick0=0, want_trace=False):
    """The launch behind ils and torch.ops.gnngls.ils: -> IlsResult, nothing raised for an instance whose matrix is not symmetric
    (its status is STATUS_ASYMMETRIC, its outputs are its inputs)."""
    B, n = _check_shapes(tour, D)
    assert cost.dtype == torch.float64 and cost.shape == (B,), f"cost shape {tuple(cost.shape)} is not [{B}]"
    kicks, kick0 = int(kicks), int(kick0)
    if u is not None:
        assert u.dtype == torch.float64 and u.shape == (B, kicks, 3), f"u shape {tuple(u.shape)} is not [{B},{kicks},3]"
        u = u.to(tour.device).contiguous()
    max_moves = min(100 * n * (kicks + 1), 2 ** 31 - 1) if max_moves is None else int(max_moves)
    dev = tour.device
    tour_out = torch.empty_like(tour)
    cost_out = torch.empty((B,), dtype=torch.float64, device=dev)
    moves = torch.zeros((B,), dtype=torch.int32, device=dev)
    accepted = torch.zeros((B,), dtype=torch.int32, device=dev)
    status = torch.zeros((B,), dtype=torch.int32, device=dev)
    trace = torch.full((B, kicks), float("nan"), dtype=torch.float64, device=dev) if want_trace else None
    f = _or_opt_entry("gnngls_ils_run")
    _lib.check(f(_lib.ptr(tour.contiguous()), _lib.ptr(cost.contiguous()), _lib.ptr(D.contiguous()), B, n, kicks, kick0, int(max_seg),
                 int(bool(reverse)), max_moves, ctypes.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), _lib.ptr(u), _lib.ptr(tour_out),
                 _lib.ptr(cost_out), _lib.ptr(moves), _lib.ptr(accepted), _lib.ptr(status), _lib.ptr(trace), _lib.current_stream()),
               "ils_run")
    return IlsResult(tour_out, cost_out, moves, accepted, status, trace)


def ils(tour, cost, D, kicks, max_seg=3, reverse=True, max_moves=None, seed=0, u=None, kick0=0, want_trace=False):
    """Iterated local search of a batch in one launch: or_opt_descent, then `kicks` times a double-bridge kick of the accepted
    tour, the same descent from the kicked tour, and the better of the two kept (include/gnngls_hip.h states the cut points,
    the kick, its delta and the acceptance rule; host.ils restates them in NumPy, bit for bit).  The cut points come from
    u [B,kicks,3] fp64 uniforms, or (None) from Philox under `seed` with the kick counter starting at kick0: a run that starts
    from an earlier run's outputs with kick0 = that run's kicks continues it exactly.  max_moves caps the applied descent moves
    of the whole run (STATUS_MOVE_CAP; None = 100 * n * (kicks + 1), clipped to int32).  kicks = 0 is or_opt_descent.
    tour [B,n+1] int32, cost [B] fp64, D [B,n,n] fp64 bitwise symmetric, n >= 4 -> IlsResult.  A matrix that is not symmetric
    raises."""
    r = ils_launch(tour, cost, D, kicks, max_seg, reverse, max_moves, seed, u, kick0, want_trace)
    bad = (r.status == STATUS_ASYMMETRIC).nonzero().flatten().tolist()
    if bad:
        _raise_asymmetric("ils", bad)
    return r


STATUS_STEP_CAP = 7                                           # GNNGLS_STATUS_STEP_CAP
_INT32_MAX = 2 ** 31 - 1


def or_opt_o2a(tour, D, pos, max_seg=3, reverse=True):
    """One best-improvement scan, for every tour of a batch in one launch, of the Or-opt candidates (s, L, rev, j) whose chain
    t[s .. s+L-1] contains the position pos[b] -- the segment-move form of the reference's relocate_o2a (operators.py:106-126),
    which it is with max_seg=1, reverse=False (include/gnngls_hip.h states the candidates and the order; host.or_opt_o2a restates
    them in NumPy, bit for bit).  tour [B,n+1] int32, D [B,n,n] fp64 bitwise symmetric, pos [B] int32 in 1..n-1 -> (delta [B]
    fp64, 0.0 when nothing qualifies; move [B,4] int32 = s, L, rev, j, -1s when none; new_tour [B,n+1] int32).  A matrix that is
    not symmetric raises."""
    B, n = _check_shapes(tour, D)
    assert pos.dtype == torch.int32 and pos.shape == (B,), f"pos shape {tuple(pos.shape)} is not [{B}]"
    if bool(((pos < 1) | (pos > n - 1)).any()):
        raise ValueError(f"or_opt_o2a: positions must be in 1..{n - 1}")
    delta = torch.empty((B,), dtype=torch.float64, device=tour.device)
    move = torch.empty((B, 4), dtype=torch.int32, device=tour.device)
    new_tour = torch.empty_like(tour)
    f = _or_opt_entry("gnngls_or_opt_o2a")
    _lib.check(f(_lib.ptr(tour.contiguous()), _lib.ptr(D.contiguous()), _lib.ptr(pos.to(tour.device).contiguous()), B, n, int(max_seg),
                 int(bool(reverse)), _lib.ptr(delta), _lib.ptr(move), _lib.ptr(new_tour), _lib.current_stream()), "or_opt_o2a")
    bad = torch.isnan(delta).nonzero().flatten().tolist()
    if bad:
        _raise_asymmetric("or_opt_o2a", bad)
    return delta, move, new_tour


@dataclass
class GuidedOrOptResult:
    tour: torch.Tensor           # [B,n+1] int32 the current tour: what a following run (iter0) starts from
    cost: torch.Tensor           # [B] fp64 its cost
    best_tour: torch.Tensor      # [B,n+1] int32
    best_cost: torch.Tensor      # [B] fp64
    moves: torch.Tensor          # [B] int32 applied moves of every kind
    steps: torch.Tensor          # [B] int32 penalisations
    status: torch.Tensor         # [B] int32 STATUS_OK, STATUS_MOVE_CAP, STATUS_STEP_CAP or (guided_or_opt_launch only) STATUS_ASYMMETRIC
    penalty: torch.Tensor        # [B,n,n] int32 the counters after the run (the caller's tensor when one was given)
    k: torch.Tensor              # [B] fp64 the penalty weight of the run
    trace_cost: torch.Tensor     # [B,trace_cap] fp64 the cost after each of the first trace_cap moves, or None
    trace_len: torch.Tensor      # [B] int32 min(moves, trace_cap)


def guided_or_opt_launch(tour, cost, D, guides, outer_iters, k=None, penalty=None, perturbation_moves=20, max_seg=3, reverse=True,
                         max_moves=None, max_steps=None, iter0=0, trace_cap=0):
    """The launch behind guided_or_opt and torch.ops.gnngls.guided_or_opt: -> GuidedOrOptResult, nothing raised for an instance
    whose matrix is not symmetric (its status is STATUS_ASYMMETRIC, its outputs are its inputs)."""
    B, n = _check_shapes(tour, D)
    dev = tour.device
    assert cost.dtype == torch.float64 and cost.shape == (B,), f"cost shape {tuple(cost.shape)} is not [{B}]"
    outer_iters, iter0, perturbation_moves, trace_cap = int(outer_iters), int(iter0), int(perturbation_moves), int(trace_cap)
    G = 0
    if guides is not None:
        assert guides.dtype == torch.float64 and guides.dim() == 4 and guides.shape[1:] == (B, n, n), \
            f"guides shape {tuple(guides.shape)} is not [G,{B},{n},{n}]"
        G = guides.shape[0]
        guides = guides.to(dev).contiguous()
    if k is None:
        # algorithms.py:137 as Python evaluates it: on the host (a tensor divided by a scalar is multiplied by its reciprocal)
        k = as_dev(0.1 * cost.cpu().numpy() / n, torch.float64).to(dev)
    assert k.dtype == torch.float64 and k.shape == (B,), f"k shape {tuple(k.shape)} is not [{B}]"
    if penalty is None:
        penalty = torch.zeros((B, n, n), dtype=torch.int32, device=dev)
    assert penalty.dtype == torch.int32 and penalty.shape == (B, n, n) and penalty.is_contiguous() and penalty.device == dev, \
        f"penalty must be a contiguous int32 [{B},{n},{n}] tensor on the tours' device (it is updated in place)"
    if max_moves is None:
        max_moves = min(100 * n * (outer_iters + 1), _INT32_MAX)
    if max_steps is None:
        max_steps = min(max(100 * max(perturbation_moves, 1) * outer_iters, 1), _INT32_MAX)
    tour_out, best_tour = torch.empty_like(tour), torch.empty_like(tour)
    cost_out, best_cost = (torch.empty((B,), dtype=torch.float64, device=dev) for _ in range(2))
    moves, steps, status, trace_len = (torch.zeros((B,), dtype=torch.int32, device=dev) for _ in range(4))
    trace = torch.zeros((B, trace_cap), dtype=torch.float64, device=dev) if trace_cap > 0 else None
    f = _or_opt_entry("gnngls_guided_or_opt_run")
    _lib.check(f(_lib.ptr(tour.contiguous()), _lib.ptr(cost.contiguous()), _lib.ptr(D.contiguous()), _lib.ptr(guides), G,
                 _lib.ptr(k.to(dev).contiguous()), _lib.ptr(penalty), B, n, outer_iters, iter0, perturbation_moves, int(max_seg),
                 int(bool(reverse)), int(max_moves), int(max_steps), _lib.ptr(tour_out), _lib.ptr(cost_out), _lib.ptr(best_tour),
                 _lib.ptr(best_cost), _lib.ptr(moves), _lib.ptr(steps), _lib.ptr(status), _lib.ptr(trace), trace_cap,
                 _lib.ptr(trace_len), _lib.current_stream()), "guided_or_opt_run")
    return GuidedOrOptResult(tour_out, cost_out, best_tour, best_cost, moves, steps, status, penalty, k, trace, trace_len)


def guided_or_opt(tour, cost, D, guides, outer_iters, k=None, penalty=None, perturbation_moves=20, max_seg=3, reverse=True,
                  max_moves=None, max_steps=None, iter0=0, trace_cap=0):
    """Guided local search over 2-opt and Or-opt of a batch in ONE launch, n <= OR_OPT_MAX_N: the reference's guided_local_search
    (algorithms.py:135-195) for `outer_iters` iterations with relocate_a2a / relocate_o2a replaced by the Or-opt scans of chains
    of 1..max_seg nodes (include/gnngls_hip.h states the definition; host.guided_or_opt restates it in NumPy, bit for bit).  With
    max_seg=1, reverse=False it is gls_run(max_outer_iters=outer_iters) bit for bit.
    tour [B,n+1] int32, cost [B] fp64, D [B,n,n] fp64 bitwise symmetric, guides [G,B,n,n] fp64 (guides[(iter0 + it) % G] steers
    iteration it), n >= 4.  k [B] fp64: the penalty weight (None: 0.1 * cost / n in fp64, the reference's); penalty [B,n,n] int32
    symmetric, updated IN PLACE (None: zeros).  max_moves caps the applied moves (STATUS_MOVE_CAP; None = 100 * n *
    (outer_iters + 1)), max_steps the penalisations (STATUS_STEP_CAP; None = 100 * perturbation_moves * outer_iters), both
    clipped to int32.  A run continues an earlier one from its .tour, .cost, .penalty and .k with iter0 = that run's
    iterations; the caller keeps the better of the two bests.  -> GuidedOrOptResult.  A matrix that is not symmetric raises."""
    r = guided_or_opt_launch(tour, cost, D, guides, outer_iters, k, penalty, perturbation_moves, max_seg, reverse, max_moves, max_steps,
                             iter0, trace_cap)
    bad = (r.status == STATUS_ASYMMETRIC).nonzero().flatten().tolist()
    if bad:
        _raise_asymmetric("guided_or_opt", bad)
    return r


ACO_MAX_N = 1024                                              # GNNGLS_ACO_MAX_N
ACO_MAX_ANTS = 256                                            # GNNGLS_ACO_MAX_ANTS


@dataclass
class AcoResult:
    best_tour: torch.Tensor      # [B,n+1] int32, closed at node 0
    best_cost: torch.Tensor      # [B] fp64 (+inf: no tour yet)
    tau: torch.Tensor            # [B,n,n] fp64 the pheromone after the run (the caller's tensor when one was given)
    iters_done: torch.Tensor     # [B] int32 completed iterations
    status: torch.Tensor         # [B] int32 STATUS_OK or (aco_launch only) SAMPLE_BAD_WEIGHTS
    trace_cost: torch.Tensor     # [B,iters] fp64 the iteration-best cost (NaN: the iteration never completed), or None
    ant_tours: torch.Tensor      # [B,ants,n+1] int32 the ants of the last iteration whose walks ran, or None
    ant_cost: torch.Tensor       # [B,ants] fp64, or None


def aco_heuristic(G, beta=2.0, kind="inverse"):
    """The heuristic matrix H of aco from an edge score G [B,n,n] where SMALLER is better, in fp64 on G's device (host.aco_heuristic
    is the same in NumPy).  kind 'inverse': G ** -beta, the classical 1 / d.  kind 'shifted', for scores that reach 0 or below
    (regret predictions, alpha): ((G - min) / (mean - min) + 0.1) ** -beta with min and mean over the off-diagonal entries of each
    instance.  The diagonal is 0.  A score that is constant over an instance has mean == min: its shifted H is 0 / 0 = NaN, which
    aco refuses (such a score says nothing; use torch.ones_like for a heuristic-free run)."""
    G = G.to(torch.float64)
    n = G.shape[-1]
    off = ~torch.eye(n, dtype=torch.bool, device=G.device)
    if kind == "inverse":
        H = G ** -float(beta)
    elif kind == "shifted":
        lo = torch.where(off, G, torch.full_like(G, float("inf"))).amin(dim=(-2, -1), keepdim=True)
        mean = torch.where(off, G, torch.zeros_like(G)).sum(dim=(-2, -1), keepdim=True) / (n * (n - 1))
        H = ((G - lo) / (mean - lo) + 0.1) ** -float(beta)
    else:
        raise ValueError(f"aco_heuristic: unknown kind {kind!r} ('inverse' or 'shifted')")
    return torch.where(off, H, torch.zeros_like(H)).contiguous()


def aco_init_tau(D, rho):
    """The start pheromone of aco, [B,n,n] fp64: every entry 1 / (rho * the cost of the instance's nearest-neighbour tour), the
    tau_max of a best tour of that cost."""
    B, n, n2 = D.shape
    assert n == n2 and D.dtype == torch.float64
    cost = tour_cost(nearest_neighbor(D), D)
    return (1.0 / (float(rho) * cost))[:, None, None].expand(B, n, n).contiguous()


def aco_launch(D, H, ants=16, iters=100, rho=0.1, min_ratio=None, gb_every=0, spread_starts=True, seed=0, u=None, iter0=0, tau=None,
               best_tour=None, best_cost=None, want_trace=False, want_ants=False):
    """The launch behind aco and torch.ops.gnngls.aco: -> AcoResult, nothing raised for an instance whose run met bad weights (its
    status is SAMPLE_BAD_WEIGHTS, its iters_done the iterations it completed)."""
    _dev()
    B, n, n2 = D.shape
    assert n == n2 and D.dtype == torch.float64
    assert H.shape == D.shape and H.dtype == torch.float64, f"H shape {tuple(H.shape)} / dtype does not match D [{B},{n},{n}] fp64"
    dev = D.device
    ants, iters, iter0 = int(ants), int(iters), int(iter0)
    if min_ratio is None:
        min_ratio = 1.0 / (2 * n)
    if u is not None:
        u = u.to(device=dev, dtype=torch.float64).contiguous()
        assert u.shape == (B, iters, ants, n - 1), f"u shape {tuple(u.shape)} is not [{B},{iters},{ants},{n - 1}]"
    if tau is None:
        tau = aco_init_tau(D, rho)
    assert tau.dtype == torch.float64 and tau.shape == (B, n, n) and tau.is_contiguous() and tau.device == dev, \
        f"tau must be a contiguous fp64 [{B},{n},{n}] tensor on D's device (it is updated in place)"
    best_tour = torch.zeros((B, n + 1), dtype=torch.int32, device=dev) if best_tour is None else best_tour.to(dev).contiguous().clone()
    best_cost = torch.full((B,), float("inf"), dtype=torch.float64, device=dev) if best_cost is None else best_cost.to(dev).contiguous().clone()
    assert best_tour.dtype == torch.int32 and best_tour.shape == (B, n + 1), f"best_tour shape {tuple(best_tour.shape)} is not [{B},{n + 1}]"
    assert best_cost.dtype == torch.float64 and best_cost.shape == (B,), f"best_cost shape {tuple(best_cost.shape)} is not [{B}]"
    iters_done, status = (torch.zeros((B,), dtype=torch.int32, device=dev) for _ in range(2))
    trace = torch.full((B, max(iters, 0)), float("nan"), dtype=torch.float64, device=dev) if want_trace else None
    ant_tours = torch.full((B, max(ants, 0), n + 1), -1, dtype=torch.int32, device=dev) if want_ants else None
    ant_cost = torch.full((B, max(ants, 0)), float("nan"), dtype=torch.float64, device=dev) if want_ants else None
    L = _lib.load()
    if not hasattr(L, "gnngls_aco_run"):
        raise _lib.GnnglsHipError("this build of libgnngls_hip.so has no gnngls_aco_run")
    _lib.check(L.gnngls_aco_run(_lib.ptr(D.contiguous()), _lib.ptr(H.contiguous()), _lib.ptr(tau), _lib.ptr(best_tour), _lib.ptr(best_cost),
                                B, n, ants, iters, iter0, float(rho), float(min_ratio), int(gb_every), int(bool(spread_starts)),
                                ctypes.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), _lib.ptr(u), _lib.ptr(iters_done), _lib.ptr(status),
                                _lib.ptr(trace), _lib.ptr(ant_tours), _lib.ptr(ant_cost), _lib.current_stream()), "aco_run")
    return AcoResult(best_tour, best_cost, tau, iters_done, status, trace, ant_tours, ant_cost)


def aco(D, H, ants=16, iters=100, rho=0.1, min_ratio=None, gb_every=0, spread_starts=True, seed=0, u=None, iter0=0, tau=None,
        best_tour=None, best_cost=None, want_trace=False, want_ants=False):
    """A MAX-MIN ant system (Stuetzle & Hoos) of a batch in ONE launch, one workgroup per instance, n <= ACO_MAX_N: `iters` times
    { `ants` sampled walks on tau * H; the cheapest ant (every gb_every-th iteration: the best tour so far) deposits 1 / cost on its
    edges after tau * (1 - rho); tau is clamped into [tau_max * min_ratio, tau_max], tau_max = 1 / (rho * best_cost) }
    (include/gnngls_hip.h states the definition; host.aco restates it in NumPy, bit for bit).
    D [B,n,n] fp64 costs; H [B,n,n] fp64 heuristic, larger = more attractive (aco_heuristic builds one from a distance, a regret
    prediction or alpha).  min_ratio None = 1 / (2 n).  spread_starts: ant a of iteration g starts at (a + g) % n, else at node 0.
    u [B,iters,ants,n-1] fp64 gives the uniforms (the run is then pinned bit for bit); None draws them on the device from Philox
    under `seed`.  tau [B,n,n] fp64 is updated IN PLACE (None: aco_init_tau(D, rho)).  A run continues an earlier one from its
    .tau, .best_tour and .best_cost with iter0 = that run's iterations, exactly.  -> AcoResult.  Weights that are no probabilities
    (NaN, negative), or costs that are not finite and positive, raise."""
    r = aco_launch(D, H, ants, iters, rho, min_ratio, gb_every, spread_starts, seed, u, iter0, tau, best_tour, best_cost, want_trace,
                   want_ants)
    bad = (r.status != 0).nonzero().flatten().tolist()
    if bad:
        raise ValueError(f"aco: instances {bad[:8]} met weights tau * H that are no probabilities (NaN, negative, infinite) or tour costs "
                         f"that are not finite and positive, after {r.iters_done[bad[:8]].tolist()} iterations (status "
                         f"{SAMPLE_BAD_WEIGHTS}): probabilities do not sum to 1")
    return r


BEAM_MAX_N = 1024                                             # GNNGLS_BEAM_MAX_N
BEAM_MAX_WIDTH = 1024                                         # GNNGLS_BEAM_MAX_WIDTH
BEAM_BAD_SCORE = 1                                            # GNNGLS_BEAM_BAD_SCORE
_BEAM_SELECT = {"score": 0, "cost": 1}                        # GNNGLS_BEAM_SELECT_*


@dataclass
class BeamResult:
    best_tour: torch.Tensor      # [B,n+1] int32, closed at the depot (-1: the instance was refused)
    best_score: torch.Tensor     # [B] fp64 the best beam's summed score
    best_cost: torch.Tensor      # [B] fp64 its tour_cost on D (NaN without D)
    n_beams: torch.Tensor        # [B] int32 final beams (below width only where the tree has fewer leaves; 0: refused)
    status: torch.Tensor         # [B] int32 STATUS_OK or (beam_search_launch only) BEAM_BAD_SCORE
    beam_tours: torch.Tensor     # [B,width,n+1] int32 every final beam by rank, rows from n_beams on -1, or None
    beam_score: torch.Tensor     # [B,width] fp64 (NaN from n_beams on), or None
    beam_cost: torch.Tensor      # [B,width] fp64 (NaN from n_beams on and without D), or None


def beam_search_workspace_bytes(B, n, width):
    """The device scratch gnngls_beam_search needs for a batch (back-pointers, a tour buffer, the visited bits beyond LDS)."""
    L = _lib.load()
    if not hasattr(L, "gnngls_beam_search"):
        raise _lib.GnnglsHipError("this build of libgnngls_hip.so has no gnngls_beam_search")
    return int(L.gnngls_beam_search_workspace_bytes(int(B), int(n), int(width)))


def beam_search_launch(S, width, depot=0, D=None, select="score", want_beams=False, workspace=None):
    """The launch behind beam_search and torch.ops.gnngls.beam_search: -> BeamResult, no synchronisation, nothing raised for a
    refused instance (its status is BEAM_BAD_SCORE).  workspace: a uint8 device tensor of at least
    beam_search_workspace_bytes(B, n, width) bytes to reuse across calls (None: allocated here)."""
    dev = _dev()
    B, n, n2 = S.shape
    assert n == n2 and S.dtype == torch.float64
    if select not in _BEAM_SELECT:
        raise ValueError(f"beam_search: unknown select {select!r} ('score' or 'cost')")
    if D is not None:
        assert D.shape == S.shape and D.dtype == torch.float64, f"D shape {tuple(D.shape)} / dtype does not match S [{B},{n},{n}] fp64"
        D = D.contiguous()
    width, depot = int(width), int(depot)
    L = _lib.load()
    if not hasattr(L, "gnngls_beam_search"):
        raise _lib.GnnglsHipError("this build of libgnngls_hip.so has no gnngls_beam_search")
    if workspace is None:
        workspace = torch.empty((max(int(L.gnngls_beam_search_workspace_bytes(B, n, width)), 16),), dtype=torch.uint8, device=dev)
    assert workspace.dtype == torch.uint8 and workspace.is_contiguous() and workspace.is_cuda, "workspace: a contiguous uint8 device tensor"
    wb = max(width, 0)
    best_tour = torch.empty((B, n + 1), dtype=torch.int32, device=dev)
    best_score, best_cost = (torch.empty((B,), dtype=torch.float64, device=dev) for _ in range(2))
    n_beams, status = (torch.empty((B,), dtype=torch.int32, device=dev) for _ in range(2))
    beam_tours = torch.empty((B, wb, n + 1), dtype=torch.int32, device=dev) if want_beams else None
    beam_score, beam_cost = ((torch.empty((B, wb), dtype=torch.float64, device=dev) for _ in range(2)) if want_beams else (None, None))
    _lib.check(L.gnngls_beam_search(_lib.ptr(S.contiguous()), _lib.ptr(D), B, n, width, depot, _BEAM_SELECT[select], _lib.ptr(best_tour),
                                    _lib.ptr(best_score), _lib.ptr(best_cost), _lib.ptr(n_beams), _lib.ptr(status), _lib.ptr(beam_tours),
                                    _lib.ptr(beam_score), _lib.ptr(beam_cost), _lib.ptr(workspace), ctypes.c_int64(workspace.numel()),
                                    _lib.current_stream()), "beam_search")
    return BeamResult(best_tour, best_score, best_cost, n_beams, status, beam_tours, beam_score, beam_cost)


def beam_search(S, width, depot=0, D=None, select="score", want_beams=False, workspace=None):
    """Beam-search decoding of a batch in ONE launch, one workgroup per instance, n <= BEAM_MAX_N, width <= BEAM_MAX_WIDTH: from
    [depot], n - 1 times { every (beam k, unvisited node j) gets key = c_k + S[last_k, j]; the `width` smallest in (key, k, j)
    are the new beams }, then every beam is closed with S[last, depot] (include/gnngls_hip.h states the definition;
    host.beam_search restates it in NumPy, bit for bit).  S [B,n,n] fp64, smaller = better (distances, alpha, a regret
    prediction, -log p); D [B,n,n] fp64 the distances or None.  select 'score': the beam of the least summed score; 'cost': the
    shortest of the final beams on D.  width = 1 is the greedy decode.  -> BeamResult (want_beams: with every final beam).  An
    instance whose S has an off-diagonal entry that is not finite raises."""
    r = beam_search_launch(S, width, depot, D, select, want_beams, workspace)
    bad = (r.status != 0).nonzero().flatten().tolist()
    if bad:
        raise ValueError(f"beam_search: instances {bad[:8]} have a score matrix with an off-diagonal entry that is NaN or infinite "
                         f"(status {BEAM_BAD_SCORE})")
    return r


GREEDY_EDGE_MAX_N = 1024                                      # GNNGLS_GREEDY_EDGE_MAX_N
GREEDY_EDGE_BAD_SCORE = 1                                     # GNNGLS_GREEDY_EDGE_BAD_SCORE
GREEDY_EDGE_STALLED = 2                                       # GNNGLS_GREEDY_EDGE_STALLED
_GREEDY_EDGE_READS = "greedy_edge_kernel reads row u of S for node u, the definition the upper triangle"


@dataclass
class GreedyEdgeResult:
    tour: torch.Tensor           # [B,n+1] int32, closed at the depot, tour[1] < tour[n-1] (-1: the instance was refused)
    score: torch.Tensor          # [B] fp64 the left-to-right sum of the edge keys along the tour
    cost: torch.Tensor           # [B] fp64 its tour_cost on D (NaN without D)
    edges: torch.Tensor          # [B,n,2] int32 the accepted edges (i < j) in acceptance order, then the closing edge, or None
    rounds: torch.Tensor         # [B] int32 rounds of simultaneous acceptances the device needed (host.greedy_edge_rounds)
    status: torch.Tensor         # [B] int32 STATUS_OK or (greedy_edge_launch only) GREEDY_EDGE_BAD_SCORE / GREEDY_EDGE_STALLED


def greedy_edge_launch(S, depot=0, D=None, want_edges=False):
    """The launch behind greedy_edge and torch.ops.gnngls.greedy_edge: -> GreedyEdgeResult, no synchronisation, nothing raised for
    a refused instance (its status is GREEDY_EDGE_BAD_SCORE).  S is NOT checked for symmetry here: the caller guarantees it (a
    matrix that is not gives an unspecified tour or GREEDY_EDGE_STALLED, never a fault)."""
    dev = _dev()
    B, n, n2 = S.shape
    assert n == n2 and S.dtype == torch.float64
    if D is not None:
        assert D.shape == S.shape and D.dtype == torch.float64, f"D shape {tuple(D.shape)} / dtype does not match S [{B},{n},{n}] fp64"
        D = D.contiguous()
    L = _lib.load()
    if not hasattr(L, "gnngls_greedy_edge"):
        raise _lib.GnnglsHipError("this build of libgnngls_hip.so has no gnngls_greedy_edge")
    tour = torch.empty((B, n + 1), dtype=torch.int32, device=dev)
    score, cost = (torch.empty((B,), dtype=torch.float64, device=dev) for _ in range(2))
    rounds, status = (torch.empty((B,), dtype=torch.int32, device=dev) for _ in range(2))
    edges = torch.empty((B, n, 2), dtype=torch.int32, device=dev) if want_edges else None
    _lib.check(L.gnngls_greedy_edge(_lib.ptr(S.contiguous()), _lib.ptr(D), B, n, int(depot), _lib.ptr(tour), _lib.ptr(score), _lib.ptr(cost),
                                    _lib.ptr(edges), _lib.ptr(rounds), _lib.ptr(status), _lib.current_stream()), "greedy_edge")
    return GreedyEdgeResult(tour, score, cost, edges, rounds, status)


def greedy_edge(S, depot=0, D=None, want_edges=False):
    """Greedy edge matching ("greedy merge") of a batch in ONE launch, one workgroup per instance, n <= GREEDY_EDGE_MAX_N: the
    edges {i, j}, i < j, in ascending (S[i,j], i, j); an edge is accepted iff both ends have degree below 2 and it closes no
    subtour; after n - 1 acceptances the path is closed (include/gnngls_hip.h states the definition; host.greedy_edge restates it
    in NumPy, bit for bit).  S [B,n,n] fp64 bitwise symmetric off the diagonal, smaller = better (distances, alpha, a regret
    prediction, -log p); D [B,n,n] fp64 the distances or None.  -> GreedyEdgeResult (want_edges: with the edges in acceptance
    order).  A matrix that is not symmetric raises before anything is launched; an instance whose S has an off-diagonal entry that
    is not finite raises after the launch."""
    assert S.dim() == 3 and S.shape[1] == S.shape[2] and S.dtype == torch.float64
    raw = S.contiguous().view(torch.int64)
    off = ~torch.eye(S.shape[1], dtype=torch.bool, device=S.device)
    bad = ((raw != raw.transpose(1, 2)) & off).flatten(1).any(dim=1).nonzero().flatten().tolist()
    if bad:
        _raise_asymmetric("greedy_edge", bad, _GREEDY_EDGE_READS)
    r = greedy_edge_launch(S, depot, D, want_edges)
    bad = (r.status == GREEDY_EDGE_BAD_SCORE).nonzero().flatten().tolist()
    if bad:
        raise ValueError(f"greedy_edge: instances {bad[:8]} have a score matrix with an off-diagonal entry that is NaN or infinite "
                         f"(status {GREEDY_EDGE_BAD_SCORE})")
    bad = (r.status != 0).nonzero().flatten().tolist()
    if bad:
        _raise_asymmetric("greedy_edge", bad, _GREEDY_EDGE_READS)
    return r


def gls_run(D, guides, init_tour, init_cost, perturbation_moves=30, first_improvement=False,
            max_outer_iters=-1, time_limit_s=0.0, watchdog_s=None, trace_cap=0, want_trace_time=False,
            want_penalty=False, penalty_bits=0, retry_overflow=True, imp_cap=0, retry_asymmetric=True):
    """guided_local_search (reference algorithms.py:135-195) for a batch of instances.

    D [B,n,n] fp64 symmetric, guides [G,B,n,n] fp64 (or None when max_outer_iters == 0 ->
    local_search only), init_tour [B,n+1] int32, init_cost [B] fp64.
    penalty_bits: 0 = auto (see include/gnngls_hip.h).  With retry_overflow (default) instances whose
    16-bit penalty counters overflowed are rerun with 32-bit counters (needs a host sync).
    (Such a rerun gets the same time_limit_s again: with penalty_bits=16 a wall-clock run can take twice the limit.)
    With retry_asymmetric (default) instances whose matrix is not bitwise symmetric (status STATUS_ASYMMETRIC: flagged on the
    device, not searched) are rerun on the global-memory store (penalty_bits = -1), which accepts any matrix (needs a host sync).
    imp_cap > 0 records the improvement trace (bounded however long the run is; see include/gnngls_hip.h).
    watchdog_s: None = time_limit_s + 5 s in wall-clock mode; in iteration-count mode a bound that scales with the
    requested work (the caller asked for exactly that many iterations, so the watchdog only catches hangs)."""
    B, n = _check_shapes(init_tour, D)
    dev = D.device
    G = 0
    if guides is not None:
        assert guides.dtype == torch.float64 and guides.dim() == 4 and guides.shape[1:] == (B, n, n)
        G = guides.shape[0]
    assert init_cost.dtype == torch.float64 and init_cost.shape == (B,)
    if watchdog_s is None:
        # iteration-count mode: ~n^2 evaluations per descent pass, tens of passes per outer iteration
        watchdog_s = (time_limit_s + 5.0) if max_outer_iters < 0 else 60.0 + 1e-7 * n * n * max(max_outer_iters, 1)
    best_tour = torch.empty_like(init_tour)
    best_cost = torch.empty((B,), dtype=torch.float64, device=dev)
    outer = torch.zeros((B,), dtype=torch.int64, device=dev)
    trace_cost = torch.zeros((B, trace_cap), dtype=torch.float64, device=dev) if trace_cap > 0 else None
    trace_time = torch.zeros((B, trace_cap), dtype=torch.float32, device=dev) if (trace_cap > 0 and want_trace_time) else None
    trace_len = torch.zeros((B,), dtype=torch.int32, device=dev)
    penalty = torch.zeros((B, n, n), dtype=torch.int32, device=dev) if want_penalty else None
    evals = torch.zeros((B,), dtype=torch.int64, device=dev)
    status = torch.zeros((B,), dtype=torch.int32, device=dev)
    imp_cost = torch.zeros((B, imp_cap), dtype=torch.float64, device=dev) if imp_cap > 0 else None
    imp_time = torch.zeros((B, imp_cap), dtype=torch.float32, device=dev) if imp_cap > 0 else None
    imp_iter = torch.zeros((B, imp_cap), dtype=torch.int64, device=dev) if imp_cap > 0 else None
    imp_len = torch.zeros((B,), dtype=torch.int32, device=dev) if imp_cap > 0 else None
    L = _lib.load()
    _lib.check(L.gnngls_gls_run(
        _lib.ptr(D), _lib.ptr(guides), G, B, n, _lib.ptr(init_tour), _lib.ptr(init_cost),
        int(perturbation_moves), int(first_improvement), int(penalty_bits), ctypes.c_int64(int(max_outer_iters)),
        float(time_limit_s), float(watchdog_s),
        _lib.ptr(best_tour), _lib.ptr(best_cost), _lib.ptr(outer),
        _lib.ptr(trace_cost), _lib.ptr(trace_time), int(trace_cap), _lib.ptr(trace_len),
        _lib.ptr(penalty), _lib.ptr(evals), _lib.ptr(status),
        _lib.ptr(imp_cost), _lib.ptr(imp_time), _lib.ptr(imp_iter), int(imp_cap), _lib.ptr(imp_len),
        _lib.current_stream()), "gls_run")
    res = GlsResult(best_tour, best_cost, outer, trace_cost, trace_time, trace_len, penalty, evals, status,
                    imp_cost, imp_time, imp_iter, imp_len)
    if retry_asymmetric and penalty_bits != -1:
        # instances whose matrix is not bitwise symmetric were flagged, not searched (the symmetric stores keep one triangle):
        # rerun them on the global-memory store, which follows the reference's index order (operators.py:25-28,97-102)
        bad = (status == STATUS_ASYMMETRIC).nonzero().flatten()
        if bad.numel() > 0:
            sub = gls_run(D[bad].contiguous(), None if guides is None else guides[:, bad].contiguous(),
                          init_tour[bad].contiguous(), init_cost[bad].contiguous(), perturbation_moves,
                          first_improvement, max_outer_iters, time_limit_s, watchdog_s, trace_cap, want_trace_time,
                          want_penalty, penalty_bits=-1, retry_overflow=False, imp_cap=imp_cap, retry_asymmetric=False)
            for name in ("best_tour", "best_cost", "outer_iters", "trace_cost", "trace_time", "trace_len", "penalty",
                         "evals", "status", "imp_cost", "imp_time", "imp_iter", "imp_len"):
                dst, src = getattr(res, name), getattr(sub, name)
                if dst is not None:
                    dst[bad] = src
    if retry_overflow and penalty_bits in (0, 16):
        bad = (status == STATUS_PENALTY_OVERFLOW).nonzero().flatten()
        if bad.numel() > 0:
            sub = gls_run(D[bad].contiguous(), None if guides is None else guides[:, bad].contiguous(),
                          init_tour[bad].contiguous(), init_cost[bad].contiguous(), perturbation_moves,
                          first_improvement, max_outer_iters, time_limit_s, watchdog_s, trace_cap, want_trace_time,
                          want_penalty, penalty_bits=32, retry_overflow=False, imp_cap=imp_cap)
            for name in ("best_tour", "best_cost", "outer_iters", "trace_cost", "trace_time", "trace_len", "penalty",
                         "evals", "status", "imp_cost", "imp_time", "imp_iter", "imp_len"):
                dst, src = getattr(res, name), getattr(sub, name)
                if dst is not None:
                    dst[bad] = src
    return res


def gls_kernel_resources(n, B=0, penalty_bits=0, first_improvement=False, trace=False):
    """-> dict(vgprs, scratch_bytes) of the kernel instantiation gls_run would launch (needs the device)."""
    v, sc = ctypes.c_int(0), ctypes.c_int(0)
    _lib.check(_lib.load().gnngls_gls_kernel_resources(int(n), int(B), int(penalty_bits), int(bool(first_improvement)), int(bool(trace)),
                                                       ctypes.cast(ctypes.byref(v), ctypes.c_void_p), ctypes.cast(ctypes.byref(sc), ctypes.c_void_p)),
               "gls_kernel_resources")
    return {"vgprs": v.value, "scratch_bytes": sc.value}


def gls_resident_capacity(n):
    return _lib.load().gnngls_gls_resident_capacity(int(n))


class gls_team_mode:
    """Experiment / test hook (gnngls_debug_set_gls_team): `with gls_team_mode(1): ...` runs gls_run with the team form of
    the perturbation phase wherever it exists, 0 never, -1 = the library's policy (B <= number of CUs).  Results are
    bit-identical either way."""

    def __init__(self, mode):
        self.mode = int(mode)

    def __enter__(self):
        _lib.check(_lib.load().gnngls_debug_set_gls_team(self.mode), "debug_set_gls_team")
        return self

    def __exit__(self, *exc):
        _lib.check(_lib.load().gnngls_debug_set_gls_team(-1), "debug_set_gls_team")
        return False


class gls_prune_mode:
    """Experiment / test hook (gnngls_debug_set_gls_prune): `with gls_prune_mode(0): ...` makes the descent evaluate every
    move of its all-to-all scans instead of the pruned candidate sets (n >= 80).  Results are bit-identical either way."""

    def __init__(self, mode):
        self.mode = int(mode)

    def __enter__(self):
        _lib.check(_lib.load().gnngls_debug_set_gls_prune(self.mode), "debug_set_gls_prune")
        return self

    def __exit__(self, *exc):
        _lib.check(_lib.load().gnngls_debug_set_gls_prune(-1), "debug_set_gls_prune")
        return False


EXEC_RECORDS = 16        # GNNGLS_EXEC_RECORDS of include/gnngls_hip.h


class executed_evals:
    """Measurement hook (gnngls_profile_set_executed_evals): `with executed_evals(B_max) as x: gls_run(...)` -> x.counts
    [B_max] int64 holds, for the LAST gls_run launch inside the block, the delta evaluations the kernel actually executed
    per instance (<= GlsResult.evals, which counts what the reference evaluates; equal where no scan is pruned; -1 where
    the run pruned on a configuration without the counting instantiations -- see include/gnngls_hip.h).  A launch inside
    the block runs the COUNTING instantiation of the kernel (2-3 % slower): measure speed outside of it."""

    def __init__(self, capacity):
        self.capacity = int(capacity)
        self.buffer = torch.zeros((EXEC_RECORDS * self.capacity,), dtype=torch.int64, device=_dev())

    def record(self, B, k):
        """Record k of the LAST launch of B instances inside the block: 0 executed evaluations, 1 shader cycles of the
        workgroup, 2 shader cycles of its serial perturbation phase, 3 penalty steps of that phase, 4 100 MHz ticks, 5 .. 14 the
        cycle account of the descent (include/gnngls_hip.h, GNNGLS_EXEC_RECORDS)."""
        return self.buffer[k * B:(k + 1) * B]

    @property
    def counts(self):
        return self.buffer[:self.capacity]

    def __enter__(self):
        _lib.check(_lib.load().gnngls_profile_set_executed_evals(_lib.ptr(self.buffer)), "profile_set_executed_evals")
        return self

    def __exit__(self, *exc):
        _lib.check(_lib.load().gnngls_profile_set_executed_evals(None), "profile_set_executed_evals")
        return False


def gls_describe_config(n, B=0, penalty_bits=0, first_improvement=False):
    """-> dict(store, threads, lds_bytes, per_cu, team, waves_per_simd[, edge_form]): exactly what gnngls_gls_run launches for
    these arguments (host-side query, gnngls_gls_describe_run).  `edge_form` (the serial perturbation phase with the tour edges
    in registers) is reported under its own key by gls_describe_run()."""
    d = gls_describe_run(n, B, penalty_bits, first_improvement)
    d.pop("edge_form")
    return d


def gls_describe_run(n, B=0, penalty_bits=0, first_improvement=False):
    vals = [ctypes.c_int(0) for _ in range(7)]
    _lib.check(_lib.load().gnngls_gls_describe_run(int(n), int(B), int(penalty_bits), int(bool(first_improvement)),
                                                   *[ctypes.cast(ctypes.byref(v), ctypes.c_void_p) for v in vals]),
               "gls_describe_run")
    names = {0: "global", 116: "lds-tri-u16", 132: "lds-tri-i32", 200: "compact"}
    return {"store": names[vals[0].value], "threads": vals[1].value, "lds_bytes": vals[2].value, "per_cu": vals[3].value,
            "team": bool(vals[5].value), "waves_per_simd": vals[4].value, "edge_form": bool(vals[6].value)}
