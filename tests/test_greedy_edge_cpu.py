"""CPU checks of greedy edge matching (gnngls_greedy_edge; include/gnngls_hip.h states the definition, gnngls_amd.host.greedy_edge
restates it, host.greedy_edge_rounds restates the parallel form the device runs).

* host.greedy_edge against an independent implementation written here (a sorted list of (key, i, j) and union-find), bit for bit.
* The round form accepts the same edges and counts 1 <= rounds <= n - 1; the chain |2^i - 2^j| needs all n - 1.
* The tie rule by hand (constant S); the orientation, the permutation, the order of the keys, the first edge.
* Refusal of one instance; the C boundary without a GPU; the Python surfaces.
"""
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gnngls_amd import host  # noqa: E402

SIZES = [3, 4, 5, 17, 64, 100]


def bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.uint64)


def euclid(rng, n):
    pos = rng.random((n, 2))
    return np.linalg.norm(pos[:, None] - pos[None], axis=2)


KINDS = {
    "euclid": lambda rng, n: euclid(rng, n),
    "nonmetric": lambda rng, n: rng.random((n, n)) * 10.0,
    "integer": lambda rng, n: rng.integers(0, 4, (n, n)).astype(np.float64),
    "constant": lambda rng, n: np.full((n, n), 0.75),
    "zeros": lambda rng, n: np.where(rng.random((n, n)) < 0.5, -0.0, 0.0),
    "negative": lambda rng, n: np.round(rng.random((n, n)) * 8.0 - 6.0, 1),
}


def independent(S, depot, D):
    """The definition, written apart from host.py: every edge as a (key, i, j) tuple, Python's sort, union-find."""
    n = S.shape[0]
    triples = sorted((float(S[i, j]) + 0.0, i, j) for i in range(n) for j in range(i + 1, n))      # x + 0.0: -0.0 -> +0.0
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    deg, adj, edges = [0] * n, {u: [] for u in range(n)}, []
    for _, i, j in triples:
        if len(edges) == n - 1:
            break
        if deg[i] < 2 and deg[j] < 2 and find(i) != find(j):
            parent[find(i)] = find(j)
            deg[i] += 1
            deg[j] += 1
            adj[i].append(j)
            adj[j].append(i)
            edges.append((i, j))
    ends = sorted(u for u in range(n) if deg[u] == 1)
    assert len(ends) == 2 and len(edges) == n - 1
    adj[ends[0]].append(ends[1])
    adj[ends[1]].append(ends[0])
    edges.append(tuple(ends))
    tour, prev, cur = [depot], depot, min(adj[depot])
    while cur != depot:
        tour.append(cur)
        prev, cur = cur, [x for x in adj[cur] if x != prev][0]
    tour.append(depot)
    score, cost = np.float64(0.0), np.float64(0.0)
    for x, y in zip(tour[:-1], tour[1:]):
        score = score + (S[min(x, y), max(x, y)] + 0.0)
        cost = cost + D[x, y]
    return tour, edges, score, cost


def cases(n):
    rng = np.random.default_rng(40 + n)
    for kind, make in KINDS.items():
        yield kind, make(rng, n), euclid(rng, n)


@pytest.mark.parametrize("n", SIZES)
def test_host_matches_an_independent_sorted_list_with_union_find(n):
    for kind, S, D in cases(n):
        for depot in sorted({0, n // 2, n - 1}):
            tour, edges, score, cost = independent(S, depot, D)
            r = host.greedy_edge(S, depot=depot, D=D)
            assert r.status == 0 and r.tour.dtype == np.int32 and r.edges.dtype == np.int32 and r.edges.shape == (n, 2), kind
            assert r.tour.tolist() == tour and r.edges.tolist() == [list(e) for e in edges], (kind, depot)
            assert bits(r.score) == bits(score) and bits(r.cost) == bits(cost), (kind, depot)
        assert np.isnan(host.greedy_edge(S).cost)                                   # no D: NaN


@pytest.mark.parametrize("n", SIZES)
def test_round_form_accepts_the_same_edges(n):
    for kind, S, D in cases(n):
        a, b = host.greedy_edge(S, depot=n - 1, D=D), host.greedy_edge_rounds(S, depot=n - 1, D=D)
        assert a.tour.tolist() == b.tour.tolist() and a.edges.tolist() == b.edges.tolist(), kind
        assert bits(a.score) == bits(b.score) and bits(a.cost) == bits(b.cost) and a.status == b.status == 0
        assert a.rounds == b.rounds and 1 <= b.rounds <= n - 1, (kind, b.rounds)


def test_only_the_upper_triangle_defines_the_keys():
    rng = np.random.default_rng(2)
    S = rng.random((20, 20))
    T = np.triu(S, 1) + np.tril(rng.random((20, 20)) * 100.0)                       # another lower triangle and diagonal
    a, b = host.greedy_edge(S, D=S), host.greedy_edge(T, D=S)
    assert a.tour.tolist() == b.tour.tolist() and a.edges.tolist() == b.edges.tolist() and bits(a.score) == bits(b.score)


def chain(n):
    p = 2.0 ** np.arange(n)
    return np.abs(p[:, None] - p[None])


def test_worst_case_chain_needs_every_round():
    # {i, i+1} has key 2^i and every other edge at i + 1 is longer than 2^i: node i + 1 prefers {i, i+1} until it is accepted, so
    # {i+1, i+2} becomes dominant only in the round after it
    n = 70
    r = host.greedy_edge_rounds(chain(n))
    assert r.rounds == n - 1 and r.tour.tolist() == list(range(n)) + [0]
    assert r.edges.tolist() == [[i, i + 1] for i in range(n - 1)] + [[0, n - 1]]
    s = host.greedy_edge(chain(n))
    assert s.rounds == n - 1 and s.tour.tolist() == r.tour.tolist() and s.edges.tolist() == r.edges.tolist()


@pytest.mark.parametrize("n", [3, 4, 5, 9, 64])
def test_constant_score_is_decided_by_the_tie_rule(n):
    # (i, j) ascending: 0 takes 1 and 2 and is full; (1, 2) would close a subtour, so 1 takes 3; then 2 takes 4, 3 takes 5, ...:
    # {k, k + 2} for every k, and the closing edge joins the last two nodes
    want = ([[0, 1]] + [[k, k + 2] for k in range(n - 2)])[:n - 1]
    assert len(want) == n - 1
    want.append([n - 2, n - 1])
    for S in (np.full((n, n), 0.75), np.zeros((n, n)), np.full((n, n), -0.0), np.full((n, n), -3.0)):
        r = host.greedy_edge(S, D=np.ones((n, n)))
        assert r.edges.tolist() == want and bits(r.cost) == bits(float(n)) and bits(r.score) == bits(S[0, 1] * n + 0.0)
        assert r.tour[1] == 1 and r.tour[-2] == 2


def test_signed_zeros_are_one_key():
    rng = np.random.default_rng(5)
    for n in (5, 17, 66):
        M = np.where(rng.random((n, n)) < 0.5, -0.0, 0.0)
        assert np.signbit(M).any() and not np.signbit(M).all()
        a, m = host.greedy_edge(np.zeros((n, n))), host.greedy_edge(M)
        assert a.edges.tolist() == m.edges.tolist() and a.tour.tolist() == m.tour.tolist() and bits(m.score) == bits(0.0)
        P = rng.integers(-1, 2, (n, n)).astype(np.float64)
        Q = np.where((P == 0) & (rng.random((n, n)) < 0.5), -0.0, P)
        a, m = host.greedy_edge(P), host.greedy_edge(Q)
        assert a.edges.tolist() == m.edges.tolist() and bits(a.score) == bits(m.score)


@pytest.mark.parametrize("n", [4, 17, 65])
def test_invariants_of_one_decode(n):
    for kind, S, D in cases(n):
        key = lambda e: (S[e[0], e[1]] + 0.0, e[0], e[1])  # noqa: E731
        first = min(((i, j) for i in range(n) for j in range(i + 1, n)), key=key)
        for depot in range(n) if n <= 17 else (0, 31, n - 1):
            r = host.greedy_edge(S, depot=depot, D=D)
            t = r.tour.tolist()
            assert t[0] == t[n] == depot and sorted(t[:-1]) == list(range(n)), kind
            assert t[1] < t[n - 1], (kind, depot)                                       # towards the smaller neighbour
            e = [tuple(x) for x in r.edges.tolist()]
            assert all(i < j for i, j in e) and len(set(e)) == n
            assert {frozenset(x) for x in e} == {frozenset(x) for x in zip(t[:-1], t[1:])}      # the edges ARE the tour's
            assert all(key(a) < key(b) for a, b in zip(e[:n - 2], e[1:n - 1])), kind         # acceptance order ascends
            assert e[0] == first, kind


def test_refusal_is_per_instance_and_ignores_the_diagonal():
    rng = np.random.default_rng(11)
    good = rng.random((6, 6))
    diag = good.copy()
    diag[np.diag_indices(6)] = np.nan
    for bad_value in (np.nan, np.inf, -np.inf):
        for where in ((4, 2), (2, 4)):
            bad = good.copy()
            bad[where] = bad_value
            for f in (host.greedy_edge, host.greedy_edge_rounds):
                r = [f(S, D=good) for S in (good, bad, diag)]
                assert [x.status for x in r] == [0, host.GREEDY_EDGE_BAD_SCORE, 0] and host.GREEDY_EDGE_BAD_SCORE == 1
                assert (r[1].tour == -1).all() and r[1].tour.shape == (7,) and (r[1].edges == -1).all() and r[1].rounds == 0
                assert np.isnan(r[1].score) and np.isnan(r[1].cost)
                assert r[0].tour.tolist() == r[2].tour.tolist() and bits(r[0].score) == bits(r[2].score)


def test_range_is_asserted():
    for f in (host.greedy_edge, host.greedy_edge_rounds):
        for S, kw in ((np.ones((4, 4)), dict(depot=4)), (np.ones((4, 4)), dict(depot=-1)), (np.ones((2, 2)), {}), (np.ones((3, 4)), {})):
            with pytest.raises(AssertionError):
                f(S, **kw)


# ---- the C ABI without a GPU -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from gnngls_amd import _lib, build
    build.build()
    return _lib.load()


def test_entry_declared_and_exported(lib):
    from gnngls_amd import _lib
    raw = ctypes.CDLL(_lib.SO)
    assert hasattr(raw, "gnngls_greedy_edge") and "gnngls_greedy_edge" in _lib.SIGNATURES and "gnngls_greedy_edge" in _lib._GREEDY_EDGE
    assert len(lib.gnngls_greedy_edge.argtypes) == 12
    assert lib.gnngls_abi_version() == 4
    header = open(os.path.join(ROOT, "include", "gnngls_hip.h")).read()
    for word in ("int gnngls_greedy_edge(", "GNNGLS_GREEDY_EDGE_MAX_N 1024", "GNNGLS_GREEDY_EDGE_BAD_SCORE 1", "(key, i, j)", "ROW u",
                 "upper triangle", "dominant"):
        assert word in header, word


def test_argument_checks_answer_before_any_device_work(lib):
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(B=1, n=5, depot=0, S=p, D=None, t=p, sc=p, co=p, e=None, ro=p, st=p):
        return lib.gnngls_greedy_edge(S, D, B, n, depot, t, sc, co, e, ro, st, None)

    hostile = [(dict(B=0), b"B=0"), (dict(n=2), b"n=2"), (dict(n=1025), b"n=1025"), (dict(n=-1), b"n=-1"), (dict(depot=5), b"depot=5"),
               (dict(depot=-1), b"depot=-1"), (dict(S=None), b"NULL"), (dict(t=None), b"NULL"), (dict(sc=None), b"NULL"),
               (dict(co=None), b"NULL"), (dict(ro=None), b"NULL"), (dict(st=None), b"NULL")]
    for kw, msg in hostile:
        assert call(**kw) == -1, kw
        err = lib.gnngls_last_error()
        assert err.startswith(b"greedy_edge:") and msg in err, (kw, err)


def test_python_surface_without_gpu():
    import torch

    from gnngls_amd import _lib, algorithms, ops, pipeline
    assert str(inspect.signature(ops.greedy_edge)) == "(S, depot=0, D=None, want_edges=False)"
    assert str(inspect.signature(ops.greedy_edge_launch)) == str(inspect.signature(ops.greedy_edge))
    assert str(inspect.signature(algorithms.greedy_edge)) == "(G, depot=0, guide='regret_pred', weight='weight')"
    assert ops.GREEDY_EDGE_MAX_N == host.GREEDY_EDGE_MAX_N == 1024 and ops.GREEDY_EDGE_BAD_SCORE == host.GREEDY_EDGE_BAD_SCORE == 1
    assert [f.name for f in ops.GreedyEdgeResult.__dataclass_fields__.values()] == ["tour", "score", "cost", "edges", "rounds", "status"]
    assert "greedy_edge" not in pipeline.INIT_TOURS
    if not torch.cuda.is_available():
        with pytest.raises(_lib.GnnglsHipError):
            ops.greedy_edge(torch.ones((1, 4, 4), dtype=torch.float64))


def test_asymmetric_score_is_refused_in_python(monkeypatch):
    import torch

    from gnngls_amd import _lib, ops

    def no_device_call(*a, **k):
        raise AssertionError("the asymmetric matrix reached the library")

    monkeypatch.setattr(_lib, "load", no_device_call)
    monkeypatch.setattr(ops, "_dev", no_device_call)
    S = torch.rand((3, 6, 6), dtype=torch.float64)
    S = S + S.transpose(1, 2)
    S[1, 2, 4] += 1.0
    S[2, 0, 5], S[2, 5, 0] = 0.0, -0.0                                              # bitwise, not by value
    S[0].fill_diagonal_(float("nan"))                                               # the diagonal does not count
    with pytest.raises(ValueError, match=r"greedy_edge: the matrices of instances \[1, 2\] are not bitwise symmetric"):
        ops.greedy_edge(S)


def test_torch_op_has_a_shape_function():
    import torch

    import gnngls_amd.torch_ops  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        S = torch.empty((3, 7, 7), dtype=torch.float64, device="cuda")
        for D in (None, S):
            out = torch.ops.gnngls.greedy_edge(S, D, 0)
            assert [tuple(o.shape) for o in out] == [(3, 8), (3,), (3,), (3, 7, 2), (3,), (3,)]
            assert [o.dtype for o in out] == [torch.int32, torch.float64, torch.float64, torch.int32, torch.int32, torch.int32]
    with pytest.raises((NotImplementedError, RuntimeError)):                   # HIP key only: no CPU kernel behind the op
        z = torch.zeros((1, 4, 4), dtype=torch.float64)
        torch.ops.gnngls.greedy_edge(z, None, 0)


def test_docs_carry_the_decoder():
    for name, words in (("README.md", ("greedy_edge_kernel", "bench_greedy_edge.py", "profiles/greedy_edge.json")),
                        ("DESIGN.md", ("greedy_edge_kernel", "dominant", "VGPR")),
                        ("INTEGRATION.md", ("ops.greedy_edge(", "torch.ops.gnngls.greedy_edge", "algorithms.greedy_edge", "gnngls_greedy_edge"))):
        text = open(os.path.join(ROOT, name)).read()
        for word in words:
            assert word in text, (name, word)
