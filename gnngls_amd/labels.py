"""Regret labels of the training data on the device: the input of scripts/train.py without LKH or Concorde.

The reference labels an instance in scripts/generate_instances.py:17-37 -> datasets.set_labels (datasets.py:23-34): Concorde's
optimal tour is the base, and every edge e off it gets regret = (cost - opt) / opt, where cost is the cost of the tour LKH
returns with e forced into it (fixed_edge_tour, gnngls/__init__.py:63-79).  Here the constrained solve is a FIXED-EDGE SEARCH
(include/gnngls_hip.h, gnngls_regret_labels): the reference's own guided_local_search on the instance with the edge's weight
lowered by M_b, for a fixed number of outer iterations -- deterministic, bit-exact with oracle/gls_oracle on that matrix.

Nothing here proves optimality, so the base is the best tour known: `nearest_neighbor` + `solve_iters` outer iterations of the
search when none is given.  When a fixed-edge search finds a tour cheaper than the base, that tour becomes the base and only the
edges of the old base that it drops get a search (the other labels stay valid: each is the true cost of a real tour holding its
edge, and they are min-merged), up to `max_rounds` rounds.  The result always satisfies: `in_solution` is a tour whose cost is
min(edge_cost), regret >= 0 everywhere and regret == 0 exactly on `in_solution`.
"""
import ctypes
import math
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib, ops

# Budgets chosen on the CPU: the oracle on D' for the 5,100 fixed-edge jobs of 30 TSP20 instances with
# exact base tours, against the Held-Karp optimum of D'.  LABEL_ITERS is the smallest budget that reproduces >= 99 % of the
# exact labels (34: 99.04 %; 30: 98.88 %; 100: 99.47 %).  The base search is one job per instance against N - n label jobs:
# 20 outer iterations from nearest_neighbor reach the optimum of 200 of 200 TSP20 instances, SOLVE_ITERS keeps a margin.
LABEL_ITERS = 34
SOLVE_ITERS = 100
PERTURBATION_MOVES = 30           # guided_local_search's default (algorithms.py:135)

STATUS_OK, STATUS_WATCHDOG, STATUS_PENALTY_OVERFLOW, STATUS_ASYMMETRIC, STATUS_EDGE_LOST = 0, 1, 2, 3, 4
STATUS_UNSETTLED = 5              # regret_labels: a search still found a cheaper base after max_rounds (labels valid, less searched)


def fixed_edge_offset(D):
    """M_b of one instance: the smallest power of two >= (2.0 n) max(D) (1.0 if that is not > 0) -- the same frexp / ldexp
    arithmetic as the device (labels_kernels.hip), so the value is identical on both sides."""
    D = np.asarray(D, dtype=np.float64)
    x = (2.0 * D.shape[0]) * float(D.max())
    if not (x > 0.0 and math.isfinite(x)):
        return 1.0
    m, e = math.frexp(x)
    return x if m == 0.5 else math.ldexp(1.0, e)


def fixed_edge_matrix(D, i, j):
    """D' of the fixed-edge search of edge (i, j): w'(i,j) = w'(j,i) = fl(D[i,j] - M)."""
    Dp = np.array(D, dtype=np.float64, copy=True)
    M = fixed_edge_offset(D)
    Dp[i, j] = D[i, j] - M
    Dp[j, i] = D[j, i] - M
    return Dp


def edge_rank(i, j, n):
    """Line-graph node of edge {i, j}: rank of (min, max) in itertools.combinations(range(n), 2) order (models.LineGraph)."""
    if i > j:
        i, j = j, i
    return i * n - i * (i + 1) // 2 + (j - i - 1)


def edge_of_rank(r, n):
    """Inverse of edge_rank."""
    i = 0
    while r >= n - 1 - i:
        r -= n - 1 - i
        i += 1
    return i, i + 1 + r


def _tour_edge_mask(tour, n):
    """[B,n+1] int32 tours -> [B,N] bool: is the line-graph node on the tour."""
    B = tour.shape[0]
    a, b = tour[:, :-1].long(), tour[:, 1:].long()
    i, j = torch.minimum(a, b), torch.maximum(a, b)
    r = i * n - i * (i + 1) // 2 + (j - i - 1)
    m = torch.zeros((B, n * (n - 1) // 2), dtype=torch.bool, device=tour.device)
    m.scatter_(1, r, True)
    return m


def _watchdog(n, iters):
    """Per search, as ops.gls_run's iteration-count mode: it only catches hangs."""
    return 60.0 + 1e-7 * n * n * max(iters, 1)


def fixed_edge_labels(D, base_tour, edge_mask=None, edge_cost=None, label_iters=LABEL_ITERS,
                      perturbation_moves=PERTURBATION_MOVES, penalty_bits=0, chunk_jobs=0, watchdog_s=None):
    """One call of gnngls_regret_labels.  D [B,n,n] fp64, base_tour [B,n+1] int32 (device).  edge_mask [B,N] bool or None
    (None: every edge off the base tour); with a mask, edge_cost [B,N] fp64 holds earlier labels and is min-merged in place.
    -> (edge_cost, regret, best_tour, best_cost, status)."""
    B, n1 = base_tour.shape
    n = n1 - 1
    assert D.dtype == torch.float64 and D.shape == (B, n, n) and base_tour.dtype == torch.int32
    N = n * (n - 1) // 2
    dev = D.device
    mask = None
    if edge_mask is None:
        edge_cost = torch.empty((B, N), dtype=torch.float64, device=dev)
    else:
        assert edge_cost is not None and edge_cost.shape == (B, N) and edge_cost.dtype == torch.float64
        mask = edge_mask.to(torch.uint8).contiguous()
    regret = torch.empty((B, N), dtype=torch.float64, device=dev)
    best_tour = torch.empty_like(base_tour)
    best_cost = torch.empty((B,), dtype=torch.float64, device=dev)
    status = torch.empty((B,), dtype=torch.int32, device=dev)
    if watchdog_s is None:
        watchdog_s = _watchdog(n, label_iters)
    _lib.check(_lib.load().gnngls_regret_labels(
        _lib.ptr(D), B, n, _lib.ptr(base_tour), _lib.ptr(mask), int(perturbation_moves), ctypes.c_int64(int(label_iters)),
        int(penalty_bits), float(watchdog_s), int(chunk_jobs), _lib.ptr(edge_cost), _lib.ptr(regret), _lib.ptr(best_tour),
        _lib.ptr(best_cost), _lib.ptr(status), _lib.current_stream()), "regret_labels")
    return edge_cost, regret, best_tour, best_cost, status


@dataclass
class LabelResult:
    tour: torch.Tensor           # [B,n+1] int32 final base tour (the cheapest tour seen)
    cost: torch.Tensor           # [B] fp64 its cost (tour_cost on D)
    in_solution: torch.Tensor    # [B,N] bool: edge on `tour` (line-graph order)
    regret: torch.Tensor         # [B,N] fp64 (edge_cost - cost) / cost
    edge_cost: torch.Tensor      # [B,N] fp64 cheapest known tour holding the edge
    rounds: torch.Tensor         # [B] int32 calls of the fixed-edge searches that labelled the instance
    status: torch.Tensor         # [B] int32 most severe status (STATUS_*)


def base_tours(D, solve_iters=SOLVE_ITERS, perturbation_moves=PERTURBATION_MOVES):
    """The default base: nearest_neighbor on D, then guided_local_search with guides=['weight'] for solve_iters outer
    iterations (algorithms.py:135-195).  -> [B,n+1] int32."""
    init = ops.nearest_neighbor(D)
    if solve_iters <= 0:
        return init
    r = ops.gls_run(D, D[None].contiguous(), init, ops.tour_cost(init, D), perturbation_moves=perturbation_moves,
                    max_outer_iters=int(solve_iters))
    bad = r.status != STATUS_OK
    if bool(bad.any()):
        raise _lib.GnnglsHipError(f"regret_labels: base search status {r.status[bad].tolist()}")
    return r.best_tour


def regret_labels(D, base_tour=None, solve_iters=SOLVE_ITERS, label_iters=LABEL_ITERS, perturbation_moves=PERTURBATION_MOVES,
                  max_rounds=3, penalty_bits=0, chunk_jobs=0):
    """Regret labels of a batch (datasets.set_labels, datasets.py:23-34).  D [B,n,n] fp64 symmetric (device or host);
    base_tour [B,n+1] or None (-> base_tours(D, solve_iters)).  -> LabelResult on D's device."""
    D = ops.as_dev(D, torch.float64)
    B, n, _ = D.shape
    if base_tour is None:
        base = base_tours(D, solve_iters, perturbation_moves)
    else:
        base = ops.as_dev(base_tour, torch.int32).clone()
    assert base.shape == (B, n + 1)
    kw = dict(label_iters=label_iters, perturbation_moves=perturbation_moves, penalty_bits=penalty_bits, chunk_jobs=chunk_jobs)
    edge_cost, regret, best_tour, best_cost, status = fixed_edge_labels(D, base, **kw)
    rounds = torch.ones((B,), dtype=torch.int32, device=D.device)
    cost = ops.tour_cost(base, D)
    while True:
        better = (best_cost < cost).nonzero().flatten()
        if better.numel() == 0:
            break
        old = base[better]
        base[better] = best_tour[better]
        # edges the old base drops get a search on the new base; at the round limit none do (flagged: labels stay valid)
        drop = _tour_edge_mask(old, n) & ~_tour_edge_mask(base[better], n)
        last = rounds[better] >= max_rounds
        drop[last] = False
        ec = edge_cost[better].contiguous()
        ec2, rg2, bt2, bc2, st2 = fixed_edge_labels(D[better].contiguous(), base[better].contiguous(), drop, ec, **kw)
        edge_cost[better], regret[better] = ec2, rg2
        cost[better] = ops.tour_cost(base[better].contiguous(), D[better].contiguous())
        best_tour[better], best_cost[better] = bt2, bc2
        status[better] = torch.maximum(status[better], st2)
        rounds[better] += (~last).to(torch.int32)
        s = status[better[last]]
        status[better[last]] = torch.where(s == STATUS_OK, torch.full_like(s, STATUS_UNSETTLED), s)
    return LabelResult(base, cost, _tour_edge_mask(base, n), regret, edge_cost, rounds, status)
