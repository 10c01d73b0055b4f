"""Host-side helpers with the names and semantics of the reference's gnngls/__init__.py (lines cited per
function).  Plain Python over the caller's networkx graph: input/output plumbing, not the hot path (the
batched device versions live in gnngls_amd.ops)."""
import functools
import operator


def _tour_edges(tour):
    return zip(tour[:-1], tour[1:])


def tour_to_edge_attribute(G, tour):
    """{edge: is it on the tour (either orientation)} for every edge of G (reference __init__.py:9-14)."""
    on_tour = {frozenset(e) for e in _tour_edges(tour)}
    return {e: frozenset(e) in on_tour for e in G.edges}


def tour_cost(G, tour, weight="weight"):
    """Sum of the edge attribute along the tour, accumulated left to right starting from the integer 0 exactly
    like the reference's `c = 0; c += w` loop (reference __init__.py:17-21) -- the fp64 summation order is part of
    the contract (the device kernels reproduce it bit for bit)."""
    return functools.reduce(operator.add, (G.edges[e][weight] for e in _tour_edges(tour)), 0)


def is_equivalent_tour(tour_a, tour_b):
    """Same cycle in either direction (reference __init__.py:24-29)."""
    return tour_a in (tour_b, tour_b[::-1])


def is_valid_tour(G, tour):
    """Starts and ends at the depot 0, visits the depot exactly twice and every other node exactly once
    (reference __init__.py:32-44)."""
    if tour[0] != 0 or tour[-1] != 0:
        return False
    return all(tour.count(v) == (2 if v == 0 else 1) for v in G.nodes)


def optimal_cost(G, weight="weight"):
    """Total weight of the edges flagged `in_solution`, in edge insertion order (reference __init__.py:55-60)."""
    return functools.reduce(operator.add, (d[weight] for _, _, d in G.edges(data=True) if d["in_solution"]), 0)


def lower_bound(G, tour=None, weight="weight", max_iters=2000):
    """A certified lower bound of G's optimal tour length: the Held-Karp 1-tree bound (oracle/one_tree.c on the device,
    gnngls_amd.ops.one_tree_bound), where the reference has only Concorde's stored optimum (optimal_cost above,
    reference __init__.py:55-60).  `tour` supplies the upper bound tour_cost(G, tour) that steers the ascent's step size
    (default: the nearest-neighbour tour on `weight` from node 0).  Typically 0.7-1 % below the optimum on uniform instances,
    the optimum itself where the ascent lands on a tour (most instances up to n ~ 20).  Returns a float."""
    import torch

    from . import ops
    from .algorithms import _attr_matrix
    D = ops.as_dev(_attr_matrix(G, weight)[None], torch.float64)
    if tour is None:
        ub = ops.tour_cost(ops.nearest_neighbor(D), D)
    else:
        ub = ops.as_dev([float(tour_cost(G, [int(v) for v in tour], weight))], torch.float64)
    return float(ops.one_tree_bound(D, ub, max_iters=max_iters, want_pi=False).bound[0])


def alpha_nearness(D, pi=None):
    """Helsgaun's alpha-nearness of one instance in NumPy fp64: the definition of include/gnngls_hip.h restated, O(n^2), the
    reference gnngls_amd.ops.alpha_nearness is compared against bit for bit (the reference package has no counterpart).
    D [n,n] symmetric, pi [n] or None (zeros) -> alpha [n,n].  Canonical weight w(i,j) = ((D[i][j] + pi[min(i,j)]) +
    pi[max(i,j)]) + 0.0; for 1 <= i < j beta(i,j) = the largest w on the path between i and j in a minimum spanning tree of
    nodes 1..n-1 (Prim: when u enters with parent p and key k, beta(u,v) = max(beta(p,v), k) for every in-tree v, beta(u,p) = k)
    and alpha = w - beta; alpha(0,j) = w(0,j) - (second smallest w(0,.)), floored at +0.0; +0.0 on the diagonal.  Every beta is
    one of the w, so the result does not depend on Prim's tie-breaks."""
    import numpy as np
    D = np.asarray(D, dtype=np.float64)
    n = D.shape[0]
    assert D.shape == (n, n) and n >= 3
    pi = np.zeros(n) if pi is None else np.asarray(pi, dtype=np.float64)
    idx = np.arange(n)
    w = ((D + pi[np.minimum.outer(idx, idx)]) + pi[np.maximum.outer(idx, idx)]) + 0.0
    beta = np.zeros((n, n))
    key = np.full(n, np.inf)
    parent = np.full(n, -1)
    outside = idx >= 1                                    # node 0 never takes part in Prim
    u = 1
    for step in range(1, n):
        if step > 1:
            u = int(np.argmin(np.where(outside, key, np.inf)))
            p, k = int(parent[u]), key[u]
            tree = ~outside
            tree[0] = False
            b = np.maximum(beta[p, tree], k)
            beta[u, tree] = b
            beta[tree, u] = b
            beta[u, p] = beta[p, u] = k
        outside[u] = False
        lower = outside & (w[u] < key)
        key[lower] = w[u, lower]
        parent[lower] = u
    alpha = w - beta
    a0 = w[0, 1:] - np.partition(w[0, 1:], 1)[1]
    alpha[0, 1:] = alpha[1:, 0] = np.where(a0 > 0, a0, 0.0)
    alpha[idx, idx] = 0.0
    return alpha


def _isclose0(delta):
    """np.isclose(0, delta) with NumPy's defaults, as the reference's acceptance rule evaluates it (operators.py:42,139)."""
    import numpy as np
    return np.abs(delta) <= 1e-8 + 1e-5 * np.abs(delta)


def or_opt_cost(tour, D, i, L, rev, j):
    """The delta of the Or-opt candidate (i, L, rev, j) (include/gnngls_hip.h states the definition): the chain S = tour[i..i+L-1]
    leaves the tour and lands, reversed if rev, at index j of the shortened tour t'.  fp64, left to right as written; for L = 1 it
    is the reference's relocate_cost (operators.py:83-103) operand by operand."""
    n = len(tour) - 1
    assert 1 <= i and i + L - 1 <= n - 1 and 1 <= L and 1 <= j <= n - L and rev in (0, 1)
    a, s1, sL, c = tour[i - 1], tour[i], tour[i + L - 1], tour[i + L]
    d = tour[j - 1] if j - 1 < i else tour[j - 1 + L]
    e = tour[j] if j < i else tour[j + L]
    if rev:
        return -D[a, s1] - D[sL, c] + D[a, c] - D[d, e] + D[d, sL] + D[s1, e]
    return -D[a, s1] - D[sL, c] + D[a, c] - D[d, e] + D[d, s1] + D[sL, e]


def or_opt(tour, i, L, rev, j):
    """The tour after the Or-opt move: t'[:j] + S (or S reversed) + t'[j:] (for L = 1 the reference's relocate,
    operators.py:76-80)."""
    tour = list(tour)
    S = tour[i:i + L]
    rest = tour[:i] + tour[i + L:]
    return rest[:j] + (S[::-1] if rev else S) + rest[j:]


def two_opt_a2a(tour, D):
    """The reference's two_opt_a2a, best improvement (operators.py:32-50), vectorised over (i, j) with its operand order:
    -> (delta, (i, j)) or (0, None)."""
    import numpy as np
    t = np.asarray(tour)
    n = len(t) - 1
    if n < 4:
        return 0, None
    D = np.asarray(D, dtype=np.float64)
    i = np.arange(1, n - 2)[:, None]
    j = np.arange(3, n)[None, :]
    a, b, c, d = t[i], t[i - 1], t[j], t[j - 1]
    delta = D[a, c] + D[b, d] - D[a, b] - D[c, d]
    ok = (j - i >= 2) & (delta < 0) & ~_isclose0(delta)
    if not ok.any():
        return 0, None
    m = delta[ok].min()
    r, col = np.argwhere(ok & (delta == m))[0]            # row-major: the first (i, j) in the reference's order
    return m, (int(r) + 1, int(col) + 3)


def or_opt_a2a(tour, D, max_seg=3, reverse=True):
    """One best-improvement scan of the Or-opt neighbourhood: every candidate (i, L, rev, j) in ascending lexicographic order,
    the reference's rule `delta < best_delta and not np.isclose(0, delta)` -- the first candidate with the smallest qualifying
    delta.  -> (delta, (i, L, rev, j)) or (0, None).  Vectorised over (i, j) per (L, rev) with the operand order of or_opt_cost;
    with max_seg=1 it is the reference's relocate_a2a (operators.py:129-147)."""
    import numpy as np
    assert 1 <= max_seg <= 3
    t = np.asarray(tour)
    n = len(t) - 1
    D = np.asarray(D, dtype=np.float64)
    best = None                                           # (delta, i, L, rev, j)
    for L in range(1, min(max_seg, n - 1) + 1):
        i = np.arange(1, n - L + 1)[:, None]              # i + L - 1 <= n - 1
        j = np.arange(1, n - L + 1)[None, :]
        a, s1, sL, c = t[i - 1], t[i], t[i + L - 1], t[i + L]
        d = t[np.where(j - 1 < i, j - 1, j - 1 + L)]
        e = t[np.where(j < i, j, j + L)]
        pre = -D[a, s1] - D[sL, c] + D[a, c] - D[d, e]
        for rev in ((0, 1) if (reverse and L >= 2) else (0,)):
            delta = (pre + D[d, sL] + D[s1, e]) if rev else (pre + D[d, s1] + D[sL, e])
            ok = (j != i) & (delta < 0) & ~_isclose0(delta)
            if not rev:
                ok &= j != i - 1                          # operators.py:135
            if not ok.any():
                continue
            m = delta[ok].min()
            r, col = np.argwhere(ok & (delta == m))[0]    # row-major: the first (i, j) of this (L, rev)
            cand = (m, int(r) + 1, L, rev, int(col) + 1)
            if best is None or cand < best:
                best = cand
    if best is None:
        return 0, None
    return best[0], best[1:]


def or_opt_descent(tour, cost, D, max_seg=3, reverse=True, max_moves=None):
    """The reference's local_search (algorithms.py:111-132), best improvement, with relocate_a2a replaced by or_opt_a2a(max_seg,
    reverse): two_opt_a2a and or_opt_a2a alternate, cost += delta after each move, until a full pass moves nothing or max_moves
    moves are applied (checked after every move; None: no cap).  -> (tour, cost, moves, cost_trace): the definition that
    gnngls_amd.ops.or_opt_descent is compared against bit for bit.  With max_seg=1, reverse=False it is local_search itself."""
    tour = [int(v) for v in tour]
    trace = []
    improved = True
    while improved:
        improved = False
        for op in (0, 1):
            if op == 0:
                delta, move = two_opt_a2a(tour, D)
            else:
                delta, move = or_opt_a2a(tour, D, max_seg, reverse)
            if move is None:
                continue
            if op == 0:
                i, j = move
                tour = tour[:i] + tour[j - 1:i - 1:-1] + tour[j:]      # operators.py:11
            else:
                tour = or_opt(tour, *move)
            cost = cost + delta
            trace.append(cost)
            improved = True
            if max_moves is not None and len(trace) >= max_moves:
                return tour, cost, len(trace), trace
    return tour, cost, len(trace), trace


def three_opt_cost(tour, D, p1, p2, p3, kind):
    """The delta of the 3-opt candidate (p1, p2, p3, kind) (include/gnngls_hip.h states the definition): the tour edges at
    positions p1 < p2 < p3 leave, the pieces B = tour[p1+1..p2] and C = tour[p2+1..p3] are reconnected between the head and the
    tail in the way `kind` names.  fp64, left to right as written: the three added edges in the table's order, then the three
    removed ones."""
    n = len(tour) - 1
    assert 0 <= p1 < p2 < p3 <= n - 1 and kind in (0, 1, 2, 3)
    a1, b1, b2, c1, c2, a2 = tour[p1], tour[p1 + 1], tour[p2], tour[p2 + 1], tour[p3], tour[p3 + 1]
    if kind == 0:
        x, y, z = D[a1, b2], D[b1, c2], D[c1, a2]
    elif kind == 1:
        x, y, z = D[a1, c1], D[c2, b1], D[b2, a2]
    elif kind == 2:
        x, y, z = D[a1, c2], D[c1, b1], D[b2, a2]
    else:
        x, y, z = D[a1, c1], D[c2, b2], D[b1, a2]
    return x + y + z - D[a1, b1] - D[b2, c1] - D[c2, a2]


def three_opt(tour, p1, p2, p3, kind):
    """The tour after the 3-opt move: H + (B reversed + C reversed | C + B | C reversed + B | C + B reversed) + T for kind 0..3,
    H = tour[0..p1], B = tour[p1+1..p2], C = tour[p2+1..p3], T = tour[p3+1..n]: the depot never moves."""
    tour = list(tour)
    H, B, C, T = tour[:p1 + 1], tour[p1 + 1:p2 + 1], tour[p2 + 1:p3 + 1], tour[p3 + 1:]
    mid = (B[::-1] + C[::-1], C + B, C[::-1] + B, C + B[::-1])[kind]
    return H + mid + T


def three_opt_a2a(tour, D):
    """One best-improvement scan of the 3-opt neighbourhood: every candidate (p1, p2, p3, kind) in ascending lexicographic order,
    the reference's rule `delta < best_delta and not np.isclose(0, delta)` -- the first candidate with the smallest qualifying
    delta.  -> (delta, (p1, p2, p3, kind)) or (0, None).  Vectorised per p1 over (p2, p3, kind) with the operand order of
    three_opt_cost."""
    import numpy as np
    t = np.asarray(tour)
    n = len(t) - 1
    D = np.asarray(D, dtype=np.float64)
    M = D[t[:, None], t[None, :]]                         # M[p, q] = D[tour[p], tour[q]]
    e = M[np.arange(n), np.arange(1, n + 1)]              # the tour edge at position p
    best = None                                           # (delta, p1, p2, p3, kind)
    for p1 in range(0, n - 2):
        p2 = np.arange(p1 + 1, n - 1)[:, None]
        p3 = np.arange(p1 + 2, n)[None, :]
        x = np.stack(np.broadcast_arrays(M[p1, p2], M[p1, p2 + 1], M[p1, p3], M[p1, p2 + 1]), axis=-1)
        y = np.stack(np.broadcast_arrays(M[p1 + 1, p3], M[p3, p1 + 1], M[p2 + 1, p1 + 1], M[p3, p2]), axis=-1)
        z = np.stack(np.broadcast_arrays(M[p2 + 1, p3 + 1], M[p2, p3 + 1], M[p2, p3 + 1], M[p1 + 1, p3 + 1]), axis=-1)
        delta = x + y + z - e[p1] - e[p2][..., None] - e[p3][..., None]
        ok = (p3 > p2)[..., None] & (delta < 0) & ~_isclose0(delta)
        if not ok.any():
            continue
        m = delta[ok].min()
        r, col, kind = np.argwhere(ok & (delta == m))[0]  # row-major: the first (p2, p3, kind) of this p1
        cand = (m, p1, int(r) + p1 + 1, int(col) + p1 + 2, int(kind))
        if best is None or cand[0] < best[0]:
            best = cand
    if best is None:
        return 0, None
    return best[0], best[1:]


def three_opt_descent(tour, cost, D, max_moves=None):
    """The reference's local_search (algorithms.py:111-132), best improvement, with relocate_a2a replaced by three_opt_a2a:
    two_opt_a2a and three_opt_a2a alternate, cost += delta after each move, until a full pass moves nothing or max_moves moves are
    applied (checked after every move; None: no cap).  -> (tour, cost, moves, cost_trace): the definition that
    gnngls_amd.ops.three_opt_descent is compared against bit for bit."""
    tour = [int(v) for v in tour]
    trace = []
    improved = True
    while improved:
        improved = False
        for op in (0, 1):
            delta, move = two_opt_a2a(tour, D) if op == 0 else three_opt_a2a(tour, D)
            if move is None:
                continue
            if op == 0:
                i, j = move
                tour = tour[:i] + tour[j - 1:i - 1:-1] + tour[j:]      # operators.py:11
            else:
                tour = three_opt(tour, *move)
            cost = cost + delta
            trace.append(cost)
            improved = True
            if max_moves is not None and len(trace) >= max_moves:
                return tour, cost, len(trace), trace
    return tour, cost, len(trace), trace


def double_bridge_cuts(u, n):
    """The cut points (p1, p2, p3) of a double-bridge kick from three uniforms in [0,1), 1 <= p1 < p2 < p3 <= n-1, n >= 4
    (include/gnngls_hip.h states the definition): with m = n - 1 each product is one fp64 multiply, truncated toward zero, then
    clamped into its range."""
    u0, u1, u2 = (float(x) for x in u)
    m = n - 1
    assert m >= 3
    p1 = 1 + min(int(u0 * (m - 2)), m - 3)
    p2 = p1 + 1 + min(int(u1 * (m - 1 - p1)), m - 2 - p1)
    p3 = p2 + 1 + min(int(u2 * (m - p2)), m - 1 - p2)
    return p1, p2, p3


def double_bridge(tour, p1, p2, p3):
    """The tour after the orientation-preserving double bridge: with A = t[0:p1], B = t[p1:p2], C = t[p2:p3], Dseg = t[p3:n] it
    is A + Dseg + C + B + [t[n]] -- A D C B: all four junctions are new, the depot never moves."""
    tour = list(tour)
    n = len(tour) - 1
    assert 1 <= p1 < p2 < p3 <= n - 1
    return tour[:p1] + tour[p3:n] + tour[p2:p3] + tour[p1:p2] + [tour[n]]


def double_bridge_cost(tour, D, p1, p2, p3):
    """The delta of that kick: the four new junctions minus the four old ones, fp64, left to right as written."""
    n = len(tour) - 1
    assert 1 <= p1 < p2 < p3 <= n - 1
    ae, bs, be, cs, ce, ds, de, z = tour[p1 - 1], tour[p1], tour[p2 - 1], tour[p2], tour[p3 - 1], tour[p3], tour[n - 1], tour[n]
    return D[ae, ds] + D[de, cs] + D[ce, bs] + D[be, z] - D[ae, bs] - D[be, cs] - D[ce, ds] - D[de, z]


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Salmon et al., SC'11) on uint64 arrays that hold 32-bit words: counter (c0, c1, c2, c3), key (k0, k1) ->
    the four output words.  The device generator (csrc/philox.h) in NumPy."""
    import numpy as np
    m32, s32 = np.uint64(0xFFFFFFFF), np.uint64(32)
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) for c in (c0, c1, c2, c3))
    k0, k1 = np.uint64(k0), np.uint64(k1)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2       # 32 x 32 bits: no overflow of 64
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & m32, (p0 >> s32) ^ c3 ^ k1, p0 & m32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m32, (k1 + np.uint64(0xBB67AE85)) & m32
    return c0, c1, c2, c3


def philox_uniforms(seed, B, K, S, b0=0, k0=0, c3=0):
    """The device's uniforms u[b,k,s] for b = b0 .. b0+B-1, k = k0 .. k0+K-1, s = 0 .. S-1: [B,K,S] fp64 in [0,1).  Key
    (seed & 0xffffffff, seed >> 32), counter (b, k, s, c3), u = ((o0 << 32 | o1) >> 11) * 2^-53.  c3 = 0 is the stream of the
    sampled walks (b, r, step, 0), c3 = 1 the stream of the double-bridge kicks (b, kick0 + k, s, 1)."""
    import numpy as np
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    b, k, s = np.meshgrid(np.arange(b0, b0 + B, dtype=np.uint64), np.arange(k0, k0 + K, dtype=np.uint64),
                          np.arange(S, dtype=np.uint64), indexing="ij")
    o0, o1, _, _ = philox4x32_10(b, k, s, np.full_like(b, c3), seed & 0xFFFFFFFF, seed >> 32)
    return (((o0 << np.uint64(32)) | o1) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


ILS_STATUS_MOVE_CAP = 6                                   # GNNGLS_STATUS_MOVE_CAP


def ils(tour, cost, D, kicks, max_seg=3, reverse=True, max_moves=None, u=None, seed=0, b=0, kick0=0):
    """Iterated local search of one instance in NumPy, the definition of include/gnngls_hip.h restated -- what gnngls_amd.ops.ils
    is compared against bit for bit.
      1. cur, cur_cost = or_opt_descent(tour, cost).
      2. for k = 0 .. kicks-1: (p1, p2, p3) = double_bridge_cuts(u[k]); cand = double_bridge(cur), cand_cost = cur_cost +
         double_bridge_cost; cand, cand_cost = or_opt_descent(cand, cand_cost); trace[k] = cand_cost; d = cand_cost - cur_cost;
         accept iff d < 0 and not np.isclose(0, d) (operators.py:42 applied to the kick): cur, cur_cost = cand, cand_cost.
      3. max_moves (None: no cap) caps the applied descent moves of the whole run, checked after every move: the descent in
         progress ends there, step 2's bookkeeping is applied to what it holds, the run ends with status ILS_STATUS_MOVE_CAP.
    u [kicks,3] uniforms in [0,1), or None: philox_uniforms(seed, 1, kicks, 3, b0=b, k0=kick0, c3=1)[0], the draws the device
    makes for instance b of a batch.  With kick0 a run continues an earlier one: K1 kicks, then K2 kicks with kick0 = K1 from
    the first run's outputs, is the run of K1 + K2 kicks.  -> (tour, cost, moves, accepted, status, trace)."""
    import numpy as np
    n = len(tour) - 1
    assert n >= 4 and kicks >= 0 and kick0 >= 0
    if u is None:
        u = philox_uniforms(seed, 1, kicks, 3, b0=b, k0=kick0, c3=1)[0]
    u = np.asarray(u, dtype=np.float64).reshape(kicks, 3)

    def left(moves):
        return None if max_moves is None else max_moves - moves

    cur, cur_cost, moves, _ = or_opt_descent(tour, cost, D, max_seg, reverse, left(0))
    accepted, trace = 0, []
    capped = max_moves is not None and moves >= max_moves
    for k in range(kicks):
        if capped:
            break
        p1, p2, p3 = double_bridge_cuts(u[k], n)
        cand_cost = cur_cost + double_bridge_cost(cur, D, p1, p2, p3)
        cand, cand_cost, m, _ = or_opt_descent(double_bridge(cur, p1, p2, p3), cand_cost, D, max_seg, reverse, left(moves))
        moves += m
        capped = max_moves is not None and moves >= max_moves
        trace.append(cand_cost)
        d = cand_cost - cur_cost
        if d < 0 and not _isclose0(d):
            cur, cur_cost = cand, cand_cost
            accepted += 1
    return cur, cur_cost, moves, accepted, ILS_STATUS_MOVE_CAP if capped else 0, trace


def two_opt_o2a(tour, D, i):
    """The reference's two_opt_o2a, best improvement (operators.py:53-73): position i against every j in 1..n-1 with
    abs(i - j) >= 2, two_opt_cost operand by operand, the rule `delta < best_delta and not np.isclose(0, delta)` -- the first j with
    the smallest qualifying delta.  -> (delta, (i, j)) or (0, None)."""
    import numpy as np
    t = np.asarray(tour)
    n = len(t) - 1
    assert 1 <= i <= n - 1
    D = np.asarray(D, dtype=np.float64)
    j = np.arange(1, n)
    lo, hi = np.minimum(i, j), np.maximum(i, j)
    a, b, c, d = t[lo], t[lo - 1], t[hi], t[hi - 1]
    delta = D[a, c] + D[b, d] - D[a, b] - D[c, d]
    ok = (np.abs(i - j) >= 2) & (delta < 0) & ~_isclose0(delta)
    if not ok.any():
        return 0, None
    m = delta[ok].min()
    return m, (i, int(j[ok & (delta == m)][0]))


def or_opt_o2a(tour, D, i, max_seg=3, reverse=True):
    """One best-improvement scan of the Or-opt candidates (s, L, rev, j) whose chain t[s .. s+L-1] contains position i:
    1 <= s <= i <= s+L-1 <= n-1, 1 <= L <= max_seg, in ascending (s, L, rev, j), with or_opt_cost's delta and or_opt_a2a's rule.
    Only j == s is skipped, in both orientations: the `rev == 0, j == s-1` skip of the all-to-all scan does not apply (the
    reference's relocate_o2a, operators.py:106-126, evaluates it, and its twin move is not in this set).  -> (delta,
    (s, L, rev, j)) or (0, None).  With max_seg=1, reverse=False it is relocate_o2a operand by operand."""
    import numpy as np
    assert 1 <= max_seg <= 3
    t = np.asarray(tour)
    n = len(t) - 1
    assert 1 <= i <= n - 1
    D = np.asarray(D, dtype=np.float64)
    best = None                                           # (delta, s, L, rev, j): ascending s, L, rev, j below, strict <
    for s in range(max(1, i - max_seg + 1), i + 1):
        for L in range(i - s + 1, max_seg + 1):
            if s + L - 1 > n - 1:
                break
            j = np.arange(1, n - L + 1)
            a, s1, sL, c = t[s - 1], t[s], t[s + L - 1], t[s + L]
            d = t[np.where(j - 1 < s, j - 1, j - 1 + L)]
            e = t[np.where(j < s, j, j + L)]
            pre = -D[a, s1] - D[sL, c] + D[a, c] - D[d, e]
            for rev in ((0, 1) if (reverse and L >= 2) else (0,)):
                delta = (pre + D[d, sL] + D[s1, e]) if rev else (pre + D[d, s1] + D[sL, e])
                ok = (j != s) & (delta < 0) & ~_isclose0(delta)
                if not ok.any():
                    continue
                m = delta[ok].min()
                if best is None or m < best[0]:
                    best = (m, s, L, rev, int(j[ok & (delta == m)][0]))
    if best is None:
        return 0, None
    return best[0], best[1:]


GUIDED_STATUS_MOVE_CAP = 6                                # GNNGLS_STATUS_MOVE_CAP
GUIDED_STATUS_STEP_CAP = 7                                # GNNGLS_STATUS_STEP_CAP


def guided_or_opt(tour, cost, D, guides, outer_iters, k, penalty, perturbation_moves=20, max_seg=3, reverse=True, max_moves=None,
                  max_steps=None, iter0=0, log=None):
    """Guided local search over 2-opt and Or-opt of one instance in NumPy, the definition of include/gnngls_hip.h restated -- what
    gnngls_amd.ops.guided_or_opt is compared against bit for bit.  It is the reference's guided_local_search
    (algorithms.py:135-195) with relocate_a2a / relocate_o2a replaced by or_opt_a2a / or_opt_o2a(max_seg, reverse), `outer_iters`
    iterations in the deadline's place, k an input (the reference's 0.1 * init_cost / n) and penalty an int32 [n,n] symmetric
    matrix updated IN PLACE.
      1. cur, cur_cost = or_opt_descent(tour, cost); best = cur.
      2. for it = 0 .. outer_iters-1: guide = guides[(iter0 + it) % G]; moves_it = 0; while moves_it < perturbation_moves:
           the penalised edge (a, b) = the first tour edge of the greatest guide[a,b] / (1 + penalty[a,b]) (lines 153-159);
           penalty[a,b] += 1, penalty[b,a] += 1; Dg = D + k * penalty, elementwise, two roundings;
           for each of a, b (in tour order) that is not the depot cur[0]: i = cur.index(node), taken once; two_opt_o2a(cur, Dg, i),
           then or_opt_o2a(cur, Dg, i) on the tour the first left; a found move replaces cur, cur_cost = the tour's cost under D
           summed left to right from 0, moves_it += 1.
         then cur, cur_cost = or_opt_descent(cur, cur_cost) on D, and best = cur on cur_cost < best_cost.
      3. max_moves (None: no cap) counts the applied moves of every kind and is checked after each; max_steps (None: no cap)
         counts penalisations and is checked before each.  A cap ends the run where it stands, the `cur_cost < best_cost`
         bookkeeping is applied to what the run holds, the status is GUIDED_STATUS_MOVE_CAP / GUIDED_STATUS_STEP_CAP.
    A run of K1 iterations, then one of K2 with iter0 = K1 from the first run's CURRENT tour, cost and penalties under the same k
    is the run of K1 + K2 iterations; the caller keeps the better of the two bests under <, ties to the earlier.
    -> (cur, cur_cost, best, best_cost, moves, steps, status, trace): trace = the cost after every applied move.  log (a list):
    gets one (it, op, move) per move of the penalty steps, op 0 = 2-opt (i, j), 1 = Or-opt (s, L, rev, j)."""
    import numpy as np
    n = len(tour) - 1
    assert n >= 4 and outer_iters >= 0 and iter0 >= 0 and perturbation_moves >= 0
    D = np.asarray(D, dtype=np.float64)
    if outer_iters > 0:
        guides = np.asarray(guides, dtype=np.float64)
        guides = guides[None] if guides.ndim == 2 else guides
    assert penalty.dtype == np.int32 and penalty.shape == (n, n)
    k = np.float64(k)

    def left(moves):
        return None if max_moves is None else max_moves - moves

    cur, cur_cost, moves, trace = or_opt_descent(tour, cost, D, max_seg, reverse, left(0))
    trace = list(trace)
    best, best_cost = cur, cur_cost
    steps = 0
    status = GUIDED_STATUS_MOVE_CAP if max_moves is not None and moves >= max_moves else 0
    for it in range(outer_iters):
        if status:
            break
        guide = guides[(iter0 + it) % len(guides)]
        moves_it = 0
        while moves_it < perturbation_moves and not status:
            if max_steps is not None and steps >= max_steps:
                status = GUIDED_STATUS_STEP_CAP
                break
            steps += 1
            t = np.asarray(cur)
            util = guide[t[:-1], t[1:]] / (1 + penalty[t[:-1], t[1:]])
            me = 0
            for p in range(1, n):                         # `util > max_util or max_util_e is None`: the first greatest
                if util[p] > util[me]:
                    me = p
            a, b = cur[me], cur[me + 1]
            penalty[a, b] += 1
            penalty[b, a] += 1
            Dg = D + k * penalty
            for node in (a, b):
                if status or node == cur[0]:
                    continue
                i = cur.index(node)
                for op in (0, 1):
                    if op == 0:
                        delta, move = two_opt_o2a(cur, Dg, i)
                    else:
                        delta, move = or_opt_o2a(cur, Dg, i, max_seg, reverse)
                    if move is None:
                        continue
                    if op == 0:
                        lo, hi = min(move), max(move)
                        cur = cur[:lo] + cur[hi - 1:lo - 1:-1] + cur[hi:]      # operators.py:11
                    else:
                        cur = or_opt(cur, *move)
                    cur_cost = 0.0
                    for x, y in zip(cur[:-1], cur[1:]):
                        cur_cost = cur_cost + D[x, y]
                    trace.append(cur_cost)
                    if log is not None:
                        log.append((it, op, move))
                    moves += 1
                    moves_it += 1
                    if max_moves is not None and moves >= max_moves:
                        status = GUIDED_STATUS_MOVE_CAP
                        break
        if not status:
            cur, cur_cost, m, tr = or_opt_descent(cur, cur_cost, D, max_seg, reverse, left(moves))
            moves += m
            trace += list(tr)
            if max_moves is not None and moves >= max_moves:
                status = GUIDED_STATUS_MOVE_CAP
        if cur_cost < best_cost:
            best, best_cost = cur, cur_cost
    return cur, cur_cost, best, best_cost, moves, steps, status, trace


ACO_STATUS_BAD_WEIGHTS = 6                                # GNNGLS_SAMPLE_BAD_WEIGHTS
ACO_MAX_N, ACO_MAX_ANTS = 1024, 256                       # GNNGLS_ACO_MAX_N, GNNGLS_ACO_MAX_ANTS


def _walk_running_sums(p):
    """The summation order of the sampled walks (include/gnngls_hip.h): p [n] fp64 with +0.0 where the node is no candidate ->
    (running sum of every node [n], total).  Node j sits on lane j % 64, slot j / 64; per slot an inclusive doubling scan over
    the 64 lanes (rounds d = 1, 2, .., 32: lane l >= d adds what lane l - d held before the round), the slots chained by
    base_0 = +0.0, base_{s+1} = base_s + scan_s[63]; total = the last base."""
    import numpy as np
    n = len(p)
    slots = (n + 63) // 64
    v = np.zeros(slots * 64, dtype=np.float64)
    v[:n] = p
    v = v.reshape(slots, 64)
    for d in (1, 2, 4, 8, 16, 32):
        old = v.copy()
        v[:, d:] = old[:, d:] + old[:, :-d]
    run = np.empty_like(v)
    base = np.float64(0.0)
    for s in range(slots):
        run[s] = base + v[s]
        base = base + v[s, 63]
    return run.reshape(-1)[:n], base


def sampled_walk(W, start, u):
    """The sampled walk of gnngls_sample_nn_tours with invert = 0, in NumPy: W [n,n] fp64 weights (W[i,j] with i the current
    node), u [n-1] uniforms -> the closed tour from `start` (a list of n+1 nodes), or None for a walk that meets weights
    np.random.choice refuses.  At every step the candidates are the unvisited nodes in ascending id with p_j = W[i,j]; if any
    p_j is infinite, p_j = 1.0 there and 0.0 elsewhere; if the sum of p is 0, every p_j = 1.0; a NaN, negative or infinite p_j or
    a total that is not finite and positive ends the walk; x = u * total and the pick is the first candidate with p_j > 0 whose
    running sum (_walk_running_sums) exceeds x, or the last candidate with p_j > 0 where rounding leaves none."""
    import numpy as np
    n = W.shape[0]
    cand = np.ones(n, dtype=bool)
    cand[start] = False
    tour, cur = [int(start)], int(start)
    with np.errstate(all="ignore"):
        for s in range(n - 1):
            p = np.where(cand, W[cur], 0.0)
            is_inf = np.isinf(p)
            if is_inf.any():
                p = np.where(is_inf, 1.0, 0.0)
            # no candidate negative or NaN: the sum in any order is 0 iff every candidate is a zero
            zero = not (p > 0).any() if (p >= 0).all() else _walk_running_sums(p)[1] == 0
            if zero:
                p = np.where(cand, 1.0, 0.0)
            if not (p >= 0).all() or np.isinf(p).any():
                return None
            run, total = _walk_running_sums(p)
            if not total > 0 or np.isinf(total):
                return None
            x = np.float64(u[s]) * total
            live = cand & (p > 0)
            over = np.flatnonzero(live & (run > x))
            cur = int(over[0]) if len(over) else int(np.flatnonzero(live)[-1])
            cand[cur] = False
            tour.append(cur)
    return tour + [int(start)]


def aco_heuristic(G, beta=2.0, kind="inverse"):
    """The heuristic matrix H of aco from an edge score G [n,n] or [B,n,n] where SMALLER is better (a distance, a regret, alpha),
    in NumPy; gnngls_amd.ops.aco_heuristic is the same on the device.  kind 'inverse': G ** -beta, the classical 1 / d.  kind
    'shifted', for scores that reach 0 or below: ((G - min) / (mean - min) + 0.1) ** -beta with min and mean over the
    off-diagonal entries of each instance (a constant score has mean == min: H is 0 / 0 = NaN, which aco refuses).  The diagonal
    is 0.  (pow is not pinned bit for bit: H is an INPUT of aco's contract.)"""
    import numpy as np
    G = np.asarray(G, dtype=np.float64)
    n = G.shape[-1]
    off = ~np.eye(n, dtype=bool)
    with np.errstate(all="ignore"):
        if kind == "inverse":
            H = G ** -float(beta)
        elif kind == "shifted":
            lo = np.where(off, G, np.inf).min(axis=(-2, -1), keepdims=True)
            mean = np.where(off, G, 0.0).sum(axis=(-2, -1), keepdims=True) / (n * (n - 1))
            H = ((G - lo) / (mean - lo) + 0.1) ** -float(beta)
        else:
            raise ValueError(f"aco_heuristic: unknown kind {kind!r} ('inverse' or 'shifted')")
    return np.where(off, H, 0.0)


def aco_init_tau(D, rho):
    """The start pheromone of aco, [n,n]: every entry 1 / (rho * the cost of the nearest-neighbour tour from node 0) -- the
    tau_max of a best tour of that cost (ties of the nearest neighbour to the lowest id, the cost summed in tour order)."""
    import numpy as np
    D = np.asarray(D, dtype=np.float64)
    n = D.shape[0]
    seen = np.zeros(n, dtype=bool)
    seen[0] = True
    tour = [0]
    for _ in range(n - 1):
        tour.append(int(np.argmin(np.where(seen, np.inf, D[tour[-1]]))))
        seen[tour[-1]] = True
    cost = np.float64(0.0)
    for x, y in zip(tour, tour[1:] + [0]):
        cost = cost + D[x, y]
    return np.full((n, n), np.float64(1.0) / (np.float64(rho) * cost))


def aco(D, H, ants=16, iters=100, rho=0.1, min_ratio=None, gb_every=0, spread_starts=True, seed=0, u=None, iter0=0, tau=None,
        best_tour=None, best_cost=None, b=0):
    """A MAX-MIN ant system of one instance in NumPy, the definition of include/gnngls_hip.h (gnngls_aco_run) restated -- what
    gnngls_amd.ops.aco is compared against bit for bit.  D, H [n,n] fp64; tau [n,n] (None: aco_init_tau(D, rho)), best_tour
    [n+1], best_cost (None: no tour yet, +inf).  For t = 0 .. iters-1, g = iter0 + t:
      1. ant a starts at (a + g) % n (spread_starts) or 0 and runs sampled_walk on tau * H with the uniforms u[t,a];
      2. its cost is that of its tour rotated to start at node 0, summed left to right;
      3. a refused walk, a cost that is not finite or a smallest cost not > 0 ends the run: status ACO_STATUS_BAD_WEIGHTS,
         iters_done = t, tau and the best pair as they were;
      4. ib = the first cheapest ant, trace[t] = cost[ib], the best pair is replaced iff cost[ib] < best_cost;
      5. X = the best tour if gb_every > 0 and (g + 1) % gb_every == 0 else ant ib's; every off-diagonal entry: tau * (1 - rho),
         + 1 / cost(X) on X's edges (both directions), clamped into [tau_max * min_ratio, tau_max], tau_max = 1 / (rho * best_cost).
    u [iters,ants,n-1] uniforms in [0,1), or None: philox_uniforms(seed, 1, iters * ants, n - 1, b0=b, k0=iter0 * ants, c3=2)
    reshaped, the draws the device makes for instance b of a batch.  min_ratio None = 1 / (2 n).  -> a namespace with tau,
    best_tour (list or None), best_cost, trace (list), iters_done, status, ant_tours [ants,n+1] int32 (rotated; -1 rows for
    refused walks) and ant_cost [ants] (NaN for those) of the last iteration whose walks ran (None when iters = 0)."""
    import types

    import numpy as np
    D, H = np.asarray(D, dtype=np.float64), np.asarray(H, dtype=np.float64)
    n = D.shape[0]
    R, K, iter0 = int(ants), int(iters), int(iter0)
    assert 3 <= n <= ACO_MAX_N and 1 <= R <= ACO_MAX_ANTS and K >= 0 and iter0 >= 0 and (iter0 + K) * R < 2 ** 32
    assert 0 < rho < 1 and gb_every >= 0
    min_ratio = np.float64(1.0 / (2 * n) if min_ratio is None else min_ratio)
    assert 0 < min_ratio <= 1
    rho = np.float64(rho)
    if u is None:
        u = philox_uniforms(seed, 1, K * R, n - 1, b0=b, k0=iter0 * R, c3=2)
    u = np.asarray(u, dtype=np.float64).reshape(K, R, n - 1)
    tau = aco_init_tau(D, rho) if tau is None else np.array(tau, dtype=np.float64)
    best = None if best_tour is None else [int(v) for v in best_tour]
    best_cost = np.float64(np.inf if best_cost is None else best_cost)
    keep = np.float64(1.0) - rho
    off = ~np.eye(n, dtype=bool)
    trace, status, done, ant_tours, ant_cost = [], 0, K, None, None
    with np.errstate(all="ignore"):
        for t in range(K):
            g = iter0 + t
            W = tau * H
            tours, ant_tours, ant_cost = [], np.full((R, n + 1), -1, dtype=np.int32), np.full(R, np.nan)
            for a in range(R):
                w = sampled_walk(W, (a + g) % n if spread_starts else 0, u[t, a])
                if w is not None:
                    z = w.index(0)
                    w = w[z:n] + w[:z] + [0]
                    c = np.float64(0.0)
                    for x, y in zip(w[:-1], w[1:]):
                        c = c + D[x, y]
                    ant_tours[a], ant_cost[a] = w, c
                tours.append(w)
            if any(w is None for w in tours) or not np.isfinite(ant_cost).all() or not ant_cost.min() > 0:
                status, done = ACO_STATUS_BAD_WEIGHTS, t
                break
            ib = int(np.argmin(ant_cost))
            trace.append(ant_cost[ib])
            if ant_cost[ib] < best_cost:
                best, best_cost = tours[ib], ant_cost[ib]
            gb = gb_every > 0 and (g + 1) % gb_every == 0
            X, xc = (best, best_cost) if gb else (tours[ib], ant_cost[ib])
            q = np.float64(1.0) / xc
            tau_max = np.float64(1.0) / (rho * best_cost)
            tau_min = tau_max * min_ratio
            on = np.zeros((n, n), dtype=bool)
            on[X[:-1], X[1:]] = True
            on[X[1:], X[:-1]] = True
            v = tau * keep
            v = np.where(on, v + q, v)
            v = np.where(v < tau_min, tau_min, v)
            v = np.where(v > tau_max, tau_max, v)
            tau = np.where(off, v, tau)
    return types.SimpleNamespace(tau=tau, best_tour=best, best_cost=best_cost, trace=trace, iters_done=done, status=status,
                                 ant_tours=ant_tours, ant_cost=ant_cost)


BEAM_MAX_N, BEAM_MAX_WIDTH = 1024, 1024                   # GNNGLS_BEAM_MAX_N, GNNGLS_BEAM_MAX_WIDTH
BEAM_STATUS_BAD_SCORE = 1                                 # GNNGLS_BEAM_BAD_SCORE


def beam_search(S, width, depot=0, D=None, select="score"):
    """Beam-search decoding of one instance in NumPy, the definition of include/gnngls_hip.h (gnngls_beam_search) restated -- what
    gnngls_amd.ops.beam_search is compared against bit for bit.  S [n,n] fp64, smaller = better; D [n,n] fp64 or None.
      step 0: one beam [depot] with c = 0.0;
      step t = 1 .. n-1: every (beam k, node j not on it) has key = c_k + S[last_k, j] (one add; a zero is taken as +0.0); the
        min(width, #candidates) smallest in (key, k, j) are the new beams, ranked in that order, c := key.  The keys are laid out
        as a [beams, n] array, so a stable argsort of its flattening IS that order (only the keys up to the width-th smallest
        value are sorted: a partition finds that value first);
      close: score = c + S[last, depot], tour = path + [depot], cost = the left-to-right sum of D along the tour;
      select 'score': the beam smallest in (score, rank); 'cost': smallest in (cost, rank), which needs D.
    An off-diagonal entry of S that is not finite refuses the instance: status BEAM_STATUS_BAD_SCORE, n_beams = 0, best_tour -1,
    NaN scores.  -> a namespace with best_tour [n+1] int32, best_score, best_cost (NaN without D), n_beams, status and all beams:
    beam_tours [width,n+1] int32, beam_score, beam_cost [width], rows from n_beams on -1 / NaN."""
    import types

    import numpy as np
    S = np.asarray(S, dtype=np.float64)
    n, W, depot = S.shape[0], int(width), int(depot)
    assert S.shape == (n, n) and 3 <= n <= BEAM_MAX_N and 1 <= W <= BEAM_MAX_WIDTH and 0 <= depot < n
    assert select in ("score", "cost") and (select == "score" or D is not None), "select='cost' needs D"
    beam_tours = np.full((W, n + 1), -1, dtype=np.int32)
    beam_score, beam_cost = np.full(W, np.nan), np.full(W, np.nan)
    if not np.isfinite(S[~np.eye(n, dtype=bool)]).all():
        return types.SimpleNamespace(best_tour=np.full(n + 1, -1, dtype=np.int32), best_score=np.float64(np.nan), best_cost=np.float64(np.nan),
                                     n_beams=0, status=BEAM_STATUS_BAD_SCORE, beam_tours=beam_tours, beam_score=beam_score, beam_cost=beam_cost)
    c = np.zeros(1)
    paths = np.full((1, 1), depot, dtype=np.int32)
    visited = np.zeros((1, n), dtype=bool)
    visited[0, depot] = True
    with np.errstate(all="ignore"):
        for t in range(1, n):
            key = c[:, None] + S[paths[:, -1]]
            key = np.where(key == 0.0, 0.0, key)
            flat = np.where(visited, np.inf, key).ravel()
            open_ = ~visited.ravel()
            m = min(W, int(open_.sum()))
            cut = np.partition(flat[open_], m - 1)[m - 1]
            cand = np.flatnonzero(open_ & (flat <= cut))            # ascending k * n + j, i.e. (k, j)
            cand = cand[np.argsort(flat[cand], kind="stable")][:m]
            k, j = cand // n, cand % n
            c = flat[cand]
            paths = np.concatenate([paths[k], j[:, None].astype(np.int32)], axis=1)
            visited = visited[k]
            visited[np.arange(m), j] = True
        nb = paths.shape[0]
        score = c + S[paths[:, -1], depot]
        score = np.where(score == 0.0, 0.0, score)
        tours = np.concatenate([paths, np.full((nb, 1), depot, dtype=np.int32)], axis=1)
        cost = np.full(nb, np.nan)
        if D is not None:
            D = np.asarray(D, dtype=np.float64)
            cost = np.zeros(nb)
            for p in range(n):                                       # tour_cost: c = 0; c += w, left to right
                cost = cost + D[tours[:, p], tours[:, p + 1]]
    v = cost if select == "cost" else score
    best = min(range(nb), key=lambda r: (v[r], r))
    beam_tours[:nb], beam_score[:nb], beam_cost[:nb] = tours, score, cost
    return types.SimpleNamespace(best_tour=tours[best].copy(), best_score=score[best], best_cost=cost[best], n_beams=nb, status=0,
                                 beam_tours=beam_tours, beam_score=beam_score, beam_cost=beam_cost)


GREEDY_EDGE_MAX_N = 1024                                  # GNNGLS_GREEDY_EDGE_MAX_N
GREEDY_EDGE_BAD_SCORE = 1                                 # GNNGLS_GREEDY_EDGE_BAD_SCORE


def _greedy_edge_keys(S):
    """-> (n, K) for greedy_edge: K[i, j] = K[j, i] = the key of {i, j} = S[min, max], a zero taken as +0.0; the diagonal +inf.
    K is None where an off-diagonal entry of S is not finite."""
    import numpy as np
    S = np.asarray(S, dtype=np.float64)
    n = S.shape[0]
    assert S.shape == (n, n) and 3 <= n <= GREEDY_EDGE_MAX_N
    if not np.isfinite(S[~np.eye(n, dtype=bool)]).all():
        return n, None
    K = np.triu(S, 1)
    K = K + K.T
    K = np.where(K == 0.0, 0.0, K)
    K[np.diag_indices(n)] = np.inf
    return n, K


def _greedy_edge_result(n, K, D, depot, nbr, accepted, rounds):
    """The closing edge, the tour from the depot and the two sums, from the n - 1 accepted edges (nbr: per node its neighbours)."""
    import types

    import numpy as np
    e0, e1 = sorted(u for u in range(n) if len(nbr[u]) == 1)
    nbr[e0].append(e1)
    nbr[e1].append(e0)
    edges = np.array(accepted + [(e0, e1)], dtype=np.int32)
    tour, prev, cur = [depot], depot, min(nbr[depot])
    for _ in range(n - 1):
        tour.append(cur)
        a, b = nbr[cur]
        prev, cur = cur, (b if a == prev else a)
    tour.append(depot)
    tour = np.array(tour, dtype=np.int32)
    score, cost = np.float64(0.0), np.float64(np.nan)
    for p in range(n):
        score = score + K[tour[p], tour[p + 1]]
    if D is not None:
        D = np.asarray(D, dtype=np.float64)
        cost = np.float64(0.0)
        for p in range(n):                                            # tour_cost: c = 0; c += w, left to right
            cost = cost + D[tour[p], tour[p + 1]]
    return types.SimpleNamespace(tour=tour, score=score, cost=cost, edges=edges, rounds=rounds, status=0)


def _greedy_edge_refused(n):
    import types

    import numpy as np
    return types.SimpleNamespace(tour=np.full(n + 1, -1, dtype=np.int32), score=np.float64(np.nan), cost=np.float64(np.nan),
                                 edges=np.full((n, 2), -1, dtype=np.int32), rounds=0, status=GREEDY_EDGE_BAD_SCORE)


def greedy_edge(S, depot=0, D=None):
    """Greedy edge matching ("greedy merge") of one instance in NumPy, the definition of include/gnngls_hip.h (gnngls_greedy_edge)
    restated -- what gnngls_amd.ops.greedy_edge is compared against bit for bit.  S [n,n] fp64, smaller = better; D [n,n] fp64 or
    None.
      keys: the key of the undirected edge {i, j}, i < j, is S[i, j] (the upper triangle alone), -0.0 and +0.0 one key; the edges are
        sorted by (key, i, j);
      acceptance: in that order, {i, j} is accepted iff deg[i] < 2, deg[j] < 2 and i, j are not the two ends of one path fragment;
        after n - 1 acceptances the two nodes of degree 1 are joined: the closing edge, the n-th;
      tour [n+1]: from depot towards the smaller-numbered of its two tour neighbours, closed at depot; score: the left-to-right sum
        of the keys along the tour from 0.0; cost: the same sum of D[tour[p], tour[p+1]], NaN without D;
      edges [n,2]: the accepted edges (i < j) in acceptance order, then the closing edge; rounds: what greedy_edge_rounds counts.
    An off-diagonal entry of S that is not finite refuses the instance: status GREEDY_EDGE_BAD_SCORE, tour and edges -1, NaN score
    and cost, rounds 0.  -> a namespace with tour, score, cost, edges, rounds, status."""
    import numpy as np
    depot = int(depot)
    n, K = _greedy_edge_keys(S)
    assert 0 <= depot < n
    if K is None:
        return _greedy_edge_refused(n)
    iu, ju = np.triu_indices(n, 1)                                    # ascending (i, j)
    order = np.argsort(K[iu, ju], kind="stable")                      # ... so a stable sort by key IS (key, i, j)
    deg, other = [0] * n, list(range(n))
    nbr = [[] for _ in range(n)]
    accepted = []
    for i, j in zip(iu[order].tolist(), ju[order].tolist()):
        if deg[i] < 2 and deg[j] < 2 and other[i] != j:
            a, b = other[i], other[j]
            other[a], other[b] = b, a
            deg[i] += 1
            deg[j] += 1
            nbr[i].append(j)
            nbr[j].append(i)
            accepted.append((i, j))
            if len(accepted) == n - 1:
                break
    return _greedy_edge_result(n, K, D, depot, nbr, accepted, greedy_edge_rounds(S, depot, None).rounds)


def greedy_edge_rounds(S, depot=0, D=None):
    """greedy_edge in the exact parallel form the device runs (greedy_edge_kernel), restated: the same namespace, `rounds` counted
    here.  Per node of degree < 2 a cached candidate cand[u] = the smallest edge {u, j} in (key, i, j) with deg[j] < 2, j != u and
    j != other[u] (the far end of u's fragment) -- for a fixed u that order is (key, j).  A round
      1. rescans the row of every end node whose cached candidate is no longer valid (validity only shrinks, so a cached minimum
         that is still valid is still the minimum);
      2. calls e = {u, v} dominant iff min(cand[u], cand[other[u]]) == e == min(cand[v], cand[other[v]]);
      3. accepts all dominant edges at once;
    until n - 1 edges are accepted.  The accepted edges, sorted by (key, i, j), are those of greedy_edge in its order: until the
    sorted pass reaches a dominant e it accepts only smaller valid edges, none of which touches an end of e's two fragments."""
    import numpy as np
    depot = int(depot)
    n, K = _greedy_edge_keys(S)
    assert 0 <= depot < n
    if K is None:
        return _greedy_edge_refused(n)
    deg, other = np.zeros(n, dtype=np.int64), np.arange(n)
    candj, candk = np.arange(n), np.full(n, np.inf)
    nbr = [[] for _ in range(n)]
    accepted, rounds = [], 0
    ids = np.arange(n)

    def edge_of(u):                                                    # cand[u] as a comparable (key, i, j)
        j = int(candj[u])
        return (candk[u], min(u, j), max(u, j))

    while len(accepted) < n - 1:
        end = deg < 2
        stale = end & ((deg[candj] >= 2) | (candj == other))
        for u in np.flatnonzero(stale).tolist():
            row = np.where(end & (ids != u) & (ids != other[u]), K[u], np.inf)
            j = int(np.argmin(row))                                    # the first of equal keys: the lowest j
            candj[u], candk[u] = j, row[j]
        found = []
        for u in np.flatnonzero(end).tolist():
            v = int(candj[u])
            if u < v and candj[v] == u:
                e = edge_of(u)
                if min(e, edge_of(int(other[u]))) == e and min(e, edge_of(int(other[v]))) == e:
                    found.append((u, v))
        assert found, "the smallest valid edge is dominant"
        for u, v in found:
            a, b = other[u], other[v]
            other[a], other[b] = b, a
            deg[u] += 1
            deg[v] += 1
            nbr[u].append(v)
            nbr[v].append(u)
            accepted.append((u, v))
        rounds += 1
    accepted.sort(key=lambda e: (K[e[0], e[1]], e[0], e[1]))
    return _greedy_edge_result(n, K, D, depot, nbr, accepted, rounds)


def fixed_edge_tour(G, e, scale=None, lkh_path=None, base_tour=None, label_iters=None, perturbation_moves=None, **kwargs):
    """A tour of G that holds edge e (reference __init__.py:63-79: LKH with e fixed).  Here: the fixed-edge search of
    gnngls_amd.labels on the device -- guided_local_search on G's weights with e's weight lowered by M, guide = those weights,
    from `base_tour` (default: G's `in_solution` tour, else labels.base_tours).  `scale`, `lkh_path` and LKH's keyword
    arguments are accepted and ignored."""
    import numpy as np
    import torch

    from . import labels, ops
    from .datasets import _tour_from_edges
    n = len(G.nodes)
    D = np.zeros((n, n), dtype=np.float64)
    for i, j, d in G.edges(data=True):
        D[i, j] = D[j, i] = d["weight"]
    if base_tour is None:
        base_tour = _tour_from_edges(G) if all("in_solution" in d for _, _, d in G.edges(data=True)) else None
    if base_tour is None:
        base_tour = labels.base_tours(ops.as_dev(D[None], torch.float64))[0].tolist()
    base_tour = [int(v) for v in base_tour]
    if frozenset(e) in {frozenset(x) for x in _tour_edges(base_tour)}:
        return base_tour
    Dp = ops.as_dev(labels.fixed_edge_matrix(D, e[0], e[1])[None], torch.float64)
    t0 = ops.as_dev([base_tour], torch.int32)
    r = ops.gls_run(Dp, Dp[None].contiguous(), t0, ops.tour_cost(t0, Dp),
                    perturbation_moves=labels.PERTURBATION_MOVES if perturbation_moves is None else perturbation_moves,
                    max_outer_iters=labels.LABEL_ITERS if label_iters is None else label_iters)
    tour = r.best_tour[0].tolist()
    if frozenset(e) not in {frozenset(x) for x in _tour_edges(tour)}:
        raise RuntimeError(f"fixed_edge_tour: the search lost edge {e} (status {int(r.status[0])})")
    return tour
