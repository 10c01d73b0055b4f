"""CPU checks of the insertion tour constructors (gnngls_insertion, gnngls_cheapest_insertion; reference algorithms.py:67-108).

* A NumPy restatement of the reference's rules (kept here; the GPU tests import it as their fuzz oracle) reproduces every fixture
  of tests/golden/insertion_*.npz bit for bit.  The fixtures are arrays captured from the reference itself by
  tests/golden/make_insertion_fixtures.py.
* The new symbols are exported with ctypes signatures, every host-side argument check answers before any device work, and the
  ABI version did not move.

The rules (reference algorithms.py:67-108, gnngls/__init__.py:17-21):
1. modes nearest / farthest: `for i in tour: for j in nodes` with a strict compare keeps the FIRST extreme pair -- the extreme
   W[i, j] with ties to the smallest tour position of i, then to the smallest j (the closed tour's second depot never wins);
2. cheapest_insertion: every position j = 1 .. len-1, cost = the left-to-right fp64 sum of ALL edge weights of the candidate
   tour, first strictly smallest wins;
3. mode random: np.random.choice on the shrinking ascending list of outside nodes, independent of the tour;
4. the tour starts as [depot, depot]; a sub-tour shorter than 2 gives None.
"""
import ctypes
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
MODES = ("nearest", "farthest", "random")
KINDS = ("euclid", "grid", "lattice", "noise")
FIXTURES = ("insertion_euclid.npz", "insertion_ties.npz", "insertion_steps.npz")


# ---- instance kinds (shared by the fixture generator and the GPU fuzz) ------------------------------------------------------
def make_instance(kind, n, rng):
    """Symmetric fp64 [n,n] matrix with a zero diagonal.
    euclid : uniform points in the unit square, Euclidean distances (np.linalg.norm, as the instance generator does)
    grid   : integer points on a small grid WITH duplicates, Manhattan distances: many exact ties and zero distances
    lattice: points on a lattice of thirds and sevenths, Manhattan distances: ties up to fp64 rounding of the rationals
    noise  : integer lattice distances + ~1e-8 symmetric noise, as tests/golden/ops_ties.npz"""
    if kind == "euclid":
        pos = rng.random((n, 2))
        D = np.array([[np.linalg.norm(pos[j] - pos[i]) for j in range(n)] for i in range(n)])
    elif kind == "grid":
        side = max(2, int(np.sqrt(n) * 0.8))
        pos = rng.integers(0, side, size=(n, 2)).astype(np.float64)
        D = np.abs(pos[:, None, 0] - pos[None, :, 0]) + np.abs(pos[:, None, 1] - pos[None, :, 1])
    elif kind == "lattice":
        side = max(2, int(np.sqrt(n)))
        pos = np.stack([rng.integers(0, side, size=n) / 3.0, rng.integers(0, side, size=n) / 7.0], axis=1)
        D = np.abs(pos[:, None, 0] - pos[None, :, 0]) + np.abs(pos[:, None, 1] - pos[None, :, 1])
    elif kind == "noise":
        base = np.triu(rng.integers(1, 4, size=(n, n)).astype(np.float64), 1)
        noise = np.triu(rng.choice([0.0, 5e-9, 1e-8, 1.00001e-8, 1.0001e-8, 2e-8, -5e-9, -1e-8], size=(n, n)), 1)
        D = base + base.T + noise + noise.T
    else:
        raise ValueError(kind)
    D = np.ascontiguousarray(D, dtype=np.float64)
    np.fill_diagonal(D, 0.0)
    assert np.array_equal(D, D.T)
    return D


# ---- the restatement ---------------------------------------------------------------------------------------------------------
def restated_cheapest_insertion(D, sub_tour, v):
    """rule 2 -> (tour, cost) or (None, None): np.cumsum is the left-to-right sum, np.argmin returns the first minimum."""
    t = np.asarray(sub_tour, dtype=np.int64)
    L = len(t)
    if L < 2:
        return None, None
    cand = np.empty((L - 1, L + 1), dtype=np.int64)
    for j in range(1, L):
        cand[j - 1, :j] = t[:j]
        cand[j - 1, j] = v
        cand[j - 1, j + 1:] = t[j:]
    edges = D[cand[:, :-1], cand[:, 1:]]
    cost = np.cumsum(np.concatenate([np.zeros((L - 1, 1)), edges], axis=1), axis=1)[:, -1]     # c = 0; c += w
    k = int(np.argmin(cost))
    return cand[k].tolist(), float(cost[k])


def restated_random_order(n, depot):
    """rule 3, with the reference's own calls (the global NumPy stream advances exactly as it does there)."""
    nodes = list(range(n))
    nodes.remove(depot)
    order = []
    while len(nodes) > 0:
        v = np.random.choice(nodes)
        nodes.remove(v)
        order.append(int(v))
    return order


def restated_insertion(D, depot, mode, order=None):
    """rules 1, 3, 4 on top of rule 2."""
    assert mode in MODES
    n = D.shape[0]
    nodes = [j for j in range(n) if j != depot]
    tour = [depot, depot]
    if mode == "random" and order is None:
        order = restated_random_order(n, depot)
    step = 0
    while nodes:
        if mode == "random":
            v = order[step]
        else:
            sub = D[np.ix_(tour, nodes)]                       # rows in tour order, columns ascending: row-major = loop order
            flat = np.argmin(sub) if mode == "nearest" else np.argmax(sub)     # first extremum
            v = nodes[int(flat) % len(nodes)]
        nodes.remove(v)
        tour, _ = restated_cheapest_insertion(D, tour, v)
        step += 1
    return tour


# ---- fixtures ---------------------------------------------------------------------------------------------------------------
def load_fixture(name):
    return np.load(os.path.join(GOLDEN, name))


def insertion_cases():
    """-> list of dict(D, depot, mode, tour, seed, next_draw) from both whole-construction fixture files."""
    out = []
    for name in FIXTURES[:2]:
        z = load_fixture(name)
        for c in range(int(z["n_cases"])):
            out.append({"D": z[f"D{int(z[f'c{c}_inst'])}"], "depot": int(z[f"c{c}_depot"]), "mode": MODES[int(z[f"c{c}_mode"])],
                        "tour": z[f"c{c}_tour"].tolist(), "seed": int(z[f"c{c}_seed"]), "next_draw": float(z[f"c{c}_next"]),
                        "id": f"{name}:{c}"})
    return out


def step_cases():
    """-> list of dict(D, sub_tour, node, tour, cost) of single cheapest_insertion steps."""
    z = load_fixture(FIXTURES[2])
    return [{"D": z[f"D{int(z[f'c{c}_inst'])}"], "sub_tour": z[f"c{c}_sub"].tolist(), "node": int(z[f"c{c}_node"]),
             "tour": z[f"c{c}_tour"].tolist(), "cost": float(z[f"c{c}_cost"]), "id": f"step:{c}"} for c in range(int(z["n_cases"]))]


def test_fixture_coverage():
    cases = insertion_cases()
    sizes = {c["D"].shape[0] for c in cases}
    assert {2, 3, 5, 8, 20, 50, 100, 200} <= sizes
    assert {c["mode"] for c in cases} == set(MODES)
    by_inst = {}
    for c in cases:
        by_inst.setdefault(c["D"].tobytes(), set()).add(c["depot"])
    assert all(len(d) == 2 for k, d in by_inst.items() if len(k) > 8 * 4)       # two depots per instance (n >= 3)
    steps = step_cases()
    assert any(len(s["sub_tour"]) == 2 for s in steps) and any(len(s["sub_tour"]) > 20 for s in steps)
    for name in FIXTURES:
        assert os.path.getsize(os.path.join(GOLDEN, name)) < (1 << 20)
    for c in cases:
        assert c["D"].dtype == np.float64 and np.array_equal(c["D"], c["D"].T)


def test_restatement_reproduces_every_fixture():
    for c in insertion_cases():
        if c["mode"] == "random":
            np.random.seed(c["seed"])
        tour = restated_insertion(c["D"], c["depot"], c["mode"])
        assert tour == c["tour"], c["id"]
        if c["mode"] == "random":
            assert np.random.random() == c["next_draw"], c["id"]
    for s in step_cases():
        tour, cost = restated_cheapest_insertion(s["D"], s["sub_tour"], s["node"])
        assert tour == s["tour"] and cost == s["cost"], s["id"]
    assert restated_cheapest_insertion(np.zeros((3, 3)), [0], 1) == (None, None)
    assert restated_cheapest_insertion(np.zeros((3, 3)), [], 1) == (None, None)


def test_delta_form_is_not_the_rule():
    """The summation rule is pinned by ordinary inputs: picking the position by w(a,v) + w(v,b) - w(a,b) gives another tour on
    some fixture (so a kernel that used it would fail the GPU tests)."""
    differs = 0
    for c in insertion_cases():
        if c["mode"] == "random" or c["D"].shape[0] < 20:
            continue
        D, depot = c["D"], c["depot"]
        nodes = [j for j in range(D.shape[0]) if j != depot]
        tour = [depot, depot]
        while nodes:
            sub = D[np.ix_(tour, nodes)]
            v = nodes[int(np.argmin(sub) if c["mode"] == "nearest" else np.argmax(sub)) % len(nodes)]
            nodes.remove(v)
            t = np.asarray(tour)
            delta = D[t[:-1], v] + D[v, t[1:]] - D[t[:-1], t[1:]]
            tour.insert(int(np.argmin(delta)) + 1, v)
        differs += tour != c["tour"]
    assert differs > 0


# ---- the C ABI without a GPU ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from gnngls_amd import _lib, build
    build.build()
    return _lib.load()


def test_entries_exported_with_signatures(lib):
    from gnngls_amd import _lib
    raw = ctypes.CDLL(_lib.SO)
    for s in ("gnngls_insertion", "gnngls_cheapest_insertion"):
        assert hasattr(raw, s) and s in _lib.SIGNATURES and s in _lib._CONSTRUCTORS
        assert len(getattr(lib, s).argtypes) == 9
    assert lib.gnngls_abi_version() == 4
    assert _lib.PROF_KINDS[-1] == "insertion" and _lib.PROF_KINDS.index("train_gat_bwd") == 17      # appended: no index moved
    header = open(os.path.join(ROOT, "include", "gnngls_hip.h")).read()
    for word in ("gnngls_insertion(", "gnngls_cheapest_insertion(", "GNNGLS_INSERT_NEAREST 0", "GNNGLS_INSERT_FARTHEST 1",
                 "GNNGLS_INSERT_GIVEN_ORDER 2", "GNNGLS_STATUS_BAD_ORDER 5", "GNNGLS_INSERTION_MAX_N 2048", "algorithms.py:82-108",
                 "algorithms.py:67-79", "NaN"):
        assert word in header, word


def test_argument_checks_answer_before_any_device_work(lib):
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    ins = lambda W, B, n, depot, mode, order, out, status: lib.gnngls_insertion(W, B, n, depot, mode, order, out, status, None)  # noqa: E731
    hostile = [
        ((None, 1, 5, 0, 0, None, p, None), -1, b"NULL"),
        ((p, 1, 5, 0, 0, None, None, None), -1, b"NULL"),
        ((p, -1, 5, 0, 0, None, p, None), -1, b"B=-1"),
        ((p, 1, 0, 0, 0, None, p, None), -1, b"n=0"),
        ((p, 1, 5, -1, 0, None, p, None), -1, b"depot=-1"),
        ((p, 1, 5, 5, 1, None, p, None), -1, b"depot=5"),
        ((p, 1, 5, 0, 3, None, p, None), -1, b"unknown mode 3"),
        ((p, 1, 5, 0, -1, None, p, None), -1, b"unknown mode -1"),
        ((p, 1, 5, 0, 2, None, p, p), -1, b"needs order and status"),
        ((p, 1, 5, 0, 2, p, p, None), -1, b"needs order and status"),
        ((p, 1, 2049, 0, 1, None, p, None), -3, b"n=2049"),
    ]
    for args, code, msg in hostile:
        assert ins(*args) == code, args
        err = lib.gnngls_last_error()
        assert err.startswith(b"insertion:") and msg in err, err
    assert ins(None, 0, 5, 0, 0, None, None, None) == 0                          # B == 0: nothing to do

    ci = lambda sub, ln, node, W, B, n, out, cost: lib.gnngls_cheapest_insertion(sub, ln, node, W, B, n, out, cost, None)  # noqa: E731
    hostile = [
        ((None, 3, p, p, 1, 5, p, p), -1, b"NULL"),
        ((p, 3, None, p, 1, 5, p, p), -1, b"NULL"),
        ((p, 3, p, None, 1, 5, p, p), -1, b"NULL"),
        ((p, 3, p, p, 1, 5, None, p), -1, b"NULL"),
        ((p, 3, p, p, 1, 5, p, None), -1, b"NULL"),
        ((p, 3, p, p, -2, 5, p, p), -1, b"B=-2"),
        ((p, 3, p, p, 1, 0, p, p), -1, b"n=0"),
        ((p, 1, p, p, 1, 5, p, p), -1, b"len=1"),
        ((p, 6, p, p, 1, 5, p, p), -1, b"len=6"),
        ((p, 3, p, p, 1, 4096, p, p), -3, b"n=4096"),
    ]
    for args, code, msg in hostile:
        assert ci(*args) == code, args
        err = lib.gnngls_last_error()
        assert err.startswith(b"cheapest_insertion:") and msg in err, err
    assert ci(None, 3, None, None, 0, 5, None, None) == 0


def test_python_surface_without_gpu():
    """Signatures and the reference's assertion text; no device is touched before the mode check."""
    import inspect

    import networkx as nx

    from gnngls_amd import algorithms, ops, pipeline
    assert str(inspect.signature(algorithms.insertion)) == "(G, depot, mode='farthest', weight='weight')"
    assert str(inspect.signature(algorithms.cheapest_insertion)) == "(G, sub_tour, n, weight='weight')"
    assert str(inspect.signature(ops.insertion)) == "(W, depot=0, mode='farthest', order=None)"
    assert str(inspect.signature(ops.cheapest_insertion)) == "(sub_tour, node, W)"
    G = nx.complete_graph(4)
    nx.set_edge_attributes(G, 1.0, "weight")
    with pytest.raises(AssertionError, match="Unknown mode: cheapest"):
        algorithms.insertion(G, 0, mode="cheapest")
    assert algorithms.cheapest_insertion(G, [0], 1) is None and algorithms.cheapest_insertion(G, [], 1) is None
    sig = inspect.signature(pipeline.solve_batch)
    assert sig.parameters["init"].default == "nearest_neighbor" and sig.parameters["init_weight"].default == "auto"
    assert list(pipeline.INIT_TOURS) == ["nearest_neighbor", "nearest_insertion", "farthest_insertion"]
    assert "out of scope" not in algorithms.__doc__.split("probabilistic")[0]
    np.random.seed(7)
    a = ops.random_order(9, 4)
    np.random.seed(7)
    assert a == restated_random_order(9, 4) and sorted(a) == [0, 1, 2, 3, 5, 6, 7, 8]


def test_torch_ops_registered():
    import torch

    import gnngls_amd.torch_ops  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        W = torch.empty((3, 7, 7), dtype=torch.float64, device="cuda")
        t = torch.ops.gnngls.insertion(W, 0, "farthest", None)
        assert t.shape == (3, 8) and t.dtype == torch.int32
        sub = torch.empty((3, 4), dtype=torch.int32, device="cuda")
        node = torch.empty((3,), dtype=torch.int32, device="cuda")
        t2, c = torch.ops.gnngls.cheapest_insertion(sub, node, W)
        assert t2.shape == (3, 5) and t2.dtype == torch.int32 and c.shape == (3,) and c.dtype == torch.float64
    with pytest.raises((NotImplementedError, RuntimeError)):                   # HIP key only: no CPU kernel behind the op
        torch.ops.gnngls.insertion(torch.zeros((1, 4, 4), dtype=torch.float64), 0, "farthest", None)
