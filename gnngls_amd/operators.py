"""Mirror of gnngls/operators.py (reference operators.py:6-147): same names, argument meaning,
return values and error behaviour, evaluated by the HIP kernels through the C ABI.

`tour` is a Python list of length n+1 with the depot at both ends, `D` an n x n array-like indexed by
node label.  a2a / o2a return `(delta, new_tour)` and never mutate their inputs.  These wrappers move
one tour per call to the GPU -- they exist for drop-in compatibility and for parity tests; the fast
path is gnngls_amd.ops / gnngls_amd.pipeline (whole batches, no host round trip per move).
"""
import numpy as np
import torch

from . import ops


def _dev(tour, D):
    t = ops.as_dev(np.asarray(tour, dtype=np.int32)[None], torch.int32)
    d = ops.as_dev(np.asarray(D, dtype=np.float64)[None], torch.float64)
    return t, d


def two_opt(tour, i, j):
    """operators.py:6-11"""
    if i == j:
        return tour
    elif j < i:
        i, j = j, i
    return tour[:i] + tour[j - 1:i - 1:-1] + tour[j:]


def two_opt_cost(tour, D, i, j):
    """operators.py:14-29"""
    if i == j:
        return 0
    t, d = _dev(tour, D)
    return ops.two_opt_delta_all(t, d)[0, i, j].item()


def _scan(op, tour, D, i, first_improvement, apply):
    t, d = _dev(tour, D)
    pos = None if i is None else torch.tensor([i], dtype=torch.int32, device=t.device)
    delta, move, _ = ops.best_move(t, d, op, pos, first_improvement)
    mi, mj = move[0].tolist()
    if mi == 0 and mj == 0:
        return 0, tour
    return delta.item(), apply(tour, mi, mj)


def two_opt_a2a(tour, D, first_improvement=False):
    """operators.py:32-50"""
    return _scan(ops.OP_TWO_OPT, tour, D, None, first_improvement, two_opt)


def two_opt_o2a(tour, D, i, first_improvement=False):
    """operators.py:53-73"""
    assert i > 0 and i < len(tour) - 1
    return _scan(ops.OP_TWO_OPT, tour, D, i, first_improvement, two_opt)


def relocate(tour, i, j):
    """operators.py:76-80"""
    new_tour = tour.copy()
    n = new_tour.pop(i)
    new_tour.insert(j, n)
    return new_tour


def relocate_cost(tour, D, i, j):
    """operators.py:83-103"""
    if i == j:
        return 0
    t, d = _dev(tour, D)
    return ops.relocate_delta_all(t, d)[0, i, j].item()


def relocate_o2a(tour, D, i, first_improvement=False):
    """operators.py:106-126"""
    assert i > 0 and i < len(tour) - 1
    return _scan(ops.OP_RELOCATE, tour, D, i, first_improvement, relocate)


def relocate_a2a(tour, D, first_improvement=False):
    """operators.py:129-147"""
    return _scan(ops.OP_RELOCATE, tour, D, None, first_improvement, relocate)


def or_opt(tour, i, L, rev, j):
    """The Or-opt move (no counterpart in the reference; for L = 1 its relocate, operators.py:76-80): the chain tour[i:i+L] leaves
    the tour and lands, reversed if rev, at index j of the shortened tour."""
    rest = tour[:i] + tour[i + L:]
    S = tour[i:i + L]
    return rest[:j] + (S[::-1] if rev else S) + rest[j:]


def or_opt_cost(tour, D, i, L, rev, j):
    """The delta of the candidate (i, L, rev, j) as include/gnngls_hip.h defines it (for L = 1 relocate_cost, operators.py:83-103).
    Four to six matrix entries: evaluated on the host by gnngls_amd.host.or_opt_cost, the definition the kernels are tested
    against; the scans below run on the GPU."""
    from . import host
    if i == j:
        return 0
    return float(host.or_opt_cost(tour, np.asarray(D, dtype=np.float64), i, L, int(bool(rev)), j))


def or_opt_a2a(tour, D, max_seg=3, reverse=True):
    """One best-improvement scan of the Or-opt neighbourhood (chains of 1..max_seg nodes, reversed too if `reverse`) in the style
    of relocate_a2a (operators.py:129-147): -> (delta, new_tour), (0, tour) when nothing qualifies."""
    t, d = _dev(tour, D)
    delta, move, _ = ops.or_opt_best_move(t, d, max_seg, reverse)
    mv = move[0].tolist()
    if mv[0] < 0:
        return 0, tour
    return delta.item(), or_opt(tour, *mv)


def three_opt(tour, p1, p2, p3, kind):
    """The 3-opt move (no counterpart in the reference): the tour edges at positions p1 < p2 < p3 leave, and B = tour[p1+1..p2]
    and C = tour[p2+1..p3] come back between the head and the tail as B reversed + C reversed (kind 0), C + B (1), C reversed + B
    (2) or C + B reversed (3)."""
    H, B, C, T = tour[:p1 + 1], tour[p1 + 1:p2 + 1], tour[p2 + 1:p3 + 1], tour[p3 + 1:]
    return H + (B[::-1] + C[::-1], C + B, C[::-1] + B, C + B[::-1])[kind] + T


def three_opt_cost(tour, D, p1, p2, p3, kind):
    """The delta of the candidate (p1, p2, p3, kind) as include/gnngls_hip.h defines it.  Six matrix entries: evaluated on the host
    by gnngls_amd.host.three_opt_cost, the definition the kernels are tested against; the scan below runs on the GPU."""
    from . import host
    return float(host.three_opt_cost(tour, np.asarray(D, dtype=np.float64), p1, p2, p3, kind))


def three_opt_a2a(tour, D):
    """One best-improvement scan of the 3-opt neighbourhood (all C(n,3) x 4 candidates) in the style of two_opt_a2a
    (operators.py:32-50): -> (delta, new_tour), (0, tour) when nothing qualifies."""
    t, d = _dev(tour, D)
    delta, move, _ = ops.three_opt_best_move(t, d)
    mv = move[0].tolist()
    if mv[0] < 0:
        return 0, tour
    return delta.item(), three_opt(tour, *mv)
