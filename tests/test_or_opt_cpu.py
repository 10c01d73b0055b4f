"""CPU checks of Or-opt (gnngls_or_opt_best_move, gnngls_or_opt_descent; the definition in include/gnngls_hip.h): the NumPy
restatement in gnngls_amd.host -- the reference of the GPU tests -- agrees with brute force, reduces to the reference's relocate
and local_search on the goldens the reference itself produced (bit for bit), keeps the stated tie rule, and ends in local
optima; and the boundary is in place: the entries are exported with ctypes signatures, argument errors are answered on the host
before any HIP call, the torch operator has a shape function.  The kernels' arithmetic is pinned on the GPU
(tests/test_or_opt_gpu.py).  Equality means equal bit patterns for every fp64 value and equal tours."""
import ctypes
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(ROOT, "tests"))

from gnngls_amd import host  # noqa: E402
from test_alpha_cpu import tie_heavy  # noqa: E402
from test_one_tree_cpu import euclid  # noqa: E402

SETTINGS = [(1, False), (1, True), (2, False), (2, True), (3, False), (3, True)]


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def tour_cost(tour, D):
    return sum(D[a, b] for a, b in zip(tour[:-1], tour[1:]))


def nn_tour(D):
    """nearest_neighbor from node 0 (reference algorithms.py:9-18), ties to the lowest id."""
    n = D.shape[0]
    tour, left = [0], np.ones(n, dtype=bool)
    left[0] = False
    while left.any():
        tour.append(int(np.argmin(np.where(left, D[tour[-1]], np.inf))))
        left[tour[-1]] = False
    return tour + [0]


def random_tour(rng, n):
    return [0] + (rng.permutation(n - 1) + 1).tolist() + [0]


def candidates(n, max_seg, reverse):
    """Every (i, L, rev, j) of the definition, in its enumeration order."""
    for i in range(1, n):
        for L in range(1, max_seg + 1):
            if i + L - 1 > n - 1:
                continue
            for rev in ((0, 1) if (reverse and L >= 2) else (0,)):
                for j in range(1, n - L + 1):
                    if j == i or (rev == 0 and j == i - 1):
                        continue
                    yield i, L, rev, j


def literal_a2a(tour, D, max_seg, reverse):
    """The scan as the definition words it: a four-deep loop in the stated order under the reference's acceptance rule."""
    best_delta, best_move = 0, None
    for i, L, rev, j in candidates(len(tour) - 1, max_seg, reverse):
        delta = host.or_opt_cost(tour, D, i, L, rev, j)
        if delta < best_delta and not np.isclose(0, delta):
            best_delta, best_move = delta, (i, L, rev, j)
    return best_delta, best_move


@pytest.mark.parametrize("n", range(5, 13))
def test_definition_against_brute_force(n):
    rng = np.random.default_rng(300 + n)
    D = euclid(rng, n)
    for _ in range(3):
        tour = random_tour(rng, n)
        old = tour_cost(tour, D)
        seen = 0
        for i, L, rev, j in candidates(n, 3, True):
            new = host.or_opt(tour, i, L, rev, j)
            assert len(new) == n + 1 and new[0] == new[-1] == 0 and sorted(new[:-1]) == list(range(n)), (tour, i, L, rev, j)
            S = tour[i:i + L]
            rest = tour[:i] + tour[i + L:]
            assert new[j:j + L] == (S[::-1] if rev else S) and new[j - 1] == rest[j - 1] and new[j + L] == rest[j]
            delta = host.or_opt_cost(tour, D, i, L, rev, j)
            assert abs(delta - (tour_cost(new, D) - old)) <= 1e-9 * old, (tour, i, L, rev, j, delta)
            seen += 1
        assert seen > 0
    assert list(candidates(3, 3, True)) == [(1, 1, 0, 2)] and len(list(candidates(4, 1, False))) == 4


@pytest.mark.parametrize("n", [8, 20, 50, 100])
def test_descent_reduces_to_the_reference_local_search(n):
    z = np.load(os.path.join(GOLDEN, f"ls_n{n}.npz"))
    tour, cost, moves, trace = host.or_opt_descent(z["fi0_init_tour"].tolist(), z["fi0_init_cost"][()], z["D"], max_seg=1, reverse=False)
    assert tour == z["fi0_tour"].tolist()
    assert bits(cost) == bits(z["fi0_cost"])
    assert moves == len(z["fi0_trace"]) and np.array_equal(bits(trace), bits(z["fi0_trace"]))


def ops_cases():
    for n in (5, 8, 20, 50, 100):
        z = np.load(os.path.join(GOLDEN, f"ops_n{n}.npz"))
        yield f"ops_n{n}", {k: z[k] for k in z.files}
    z = np.load(os.path.join(GOLDEN, "ops_ties.npz"))
    for c in range(int(z["n_cases"])):
        yield f"ops_ties c{c}", {k[len(f"c{c}_"):]: z[k] for k in z.files if k.startswith(f"c{c}_")}


def test_single_node_moves_equal_the_relocate_goldens():
    count = 0
    for what, g in ops_cases():
        tour, D, table = g["tour"].tolist(), g["D"], g["relocate_table"]
        n = len(tour) - 1
        for i in range(1, n):
            for j in range(1, n):
                if i == j or i - j == 1:                       # operators.py:134-136
                    continue
                assert bits(host.or_opt_cost(tour, D, i, 1, 0, j)) == bits(table[i, j]), (what, i, j)
                count += 1
        delta, move = host.or_opt_a2a(tour, D, max_seg=1, reverse=False)
        assert bits(delta) == bits(g["relocate_a2a_fi0_delta"]), what
        new = tour if move is None else host.or_opt(tour, *move)
        assert new == g["relocate_a2a_fi0_tour"].tolist(), what
        # reversal has nothing to enumerate at one node
        assert host.or_opt_a2a(tour, D, max_seg=1, reverse=True) == (delta, move)
    assert count > 10000


@pytest.mark.parametrize("n", [6, 12, 20, 33])
def test_tie_rule_equals_the_literal_loop(n):
    rng = np.random.default_rng(4000 + n)
    ties = 0
    for _ in range(4):
        D = tie_heavy(rng, n)
        tour = random_tour(rng, n)
        for max_seg, reverse in SETTINGS:
            want = literal_a2a(tour, D, max_seg, reverse)
            got = host.or_opt_a2a(tour, D, max_seg, reverse)
            assert got[1] == want[1] and bits(got[0]) == bits(want[0]), (n, max_seg, reverse, got, want)
            if want[1] is not None:
                ties += sum(host.or_opt_cost(tour, D, *c) == want[0] for c in candidates(n, max_seg, reverse)) > 1
    assert ties > 0 or n < 12                                   # the matrices do produce tied minima
    # and on tie-free instances
    D = euclid(rng, n)
    tour = random_tour(rng, n)
    for max_seg, reverse in SETTINGS:
        want = literal_a2a(tour, D, max_seg, reverse)
        got = host.or_opt_a2a(tour, D, max_seg, reverse)
        assert got[1] == want[1] and bits(got[0]) == bits(want[0])


@pytest.mark.parametrize("n", [5, 20, 64, 100])
def test_descent_ends_in_a_local_optimum_of_both_scans(n):
    for s, D in enumerate((euclid(np.random.default_rng(1000 + n), n), tie_heavy(np.random.default_rng(2000 + n), n))):
        init = nn_tour(D)
        for max_seg, reverse in SETTINGS:
            tour, cost, moves, trace = host.or_opt_descent(init, tour_cost(init, D), D, max_seg, reverse)
            assert host.two_opt_a2a(tour, D) == (0, None) and host.or_opt_a2a(tour, D, max_seg, reverse) == (0, None)
            assert moves == len(trace) and sorted(tour[:-1]) == list(range(n)) and tour[0] == tour[-1] == 0
            assert abs(cost - tour_cost(tour, D)) <= 1e-9 * cost and all(b < a for a, b in zip([tour_cost(init, D)] + trace, trace))
            # the cap is checked after every move: the first k moves of the same trajectory
            if moves >= 2:
                t2, c2, m2, tr2 = host.or_opt_descent(init, tour_cost(init, D), D, max_seg, reverse, max_moves=2)
                assert m2 == 2 and np.array_equal(bits(tr2), bits(trace[:2])) and bits(c2) == bits(trace[1])


@pytest.fixture(scope="module")
def lib():
    from gnngls_amd import _lib, build
    build.build()
    return _lib.load()


def test_entries_exported_with_signatures(lib):
    from gnngls_amd import _lib
    raw = ctypes.CDLL(_lib.SO)
    for name, nargs in (("gnngls_or_opt_best_move", 10), ("gnngls_or_opt_descent", 15)):
        assert hasattr(raw, name) and name in _lib.SIGNATURES
        assert len(getattr(lib, name).argtypes) == nargs
    assert lib.gnngls_abi_version() == 4
    h = open(os.path.join(ROOT, "include", "gnngls_hip.h")).read()
    for word in ("gnngls_or_opt_best_move(", "gnngls_or_opt_descent(", "GNNGLS_OR_OPT_MAX_N 1024", "GNNGLS_STATUS_MOVE_CAP 6",
                 "-D[a,s1] - D[sL,c] + D[a,c] - D[d,e] + D[d,sL] + D[s1,e]", "(i, L, rev, j)"):
        assert word in h, word


def test_argument_checks_answer_before_any_device_work(lib):
    """No GPU here: an entry that reached a HIP call would answer GNNGLS_ERR_HIP (-2), not these codes."""
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    # tour, D, B, n, max_seg, reverse, delta, move, new_tour
    scan = [
        ((None, p, 1, 5, 3, 1, p, p, p), -1, b"NULL"),
        ((p, None, 1, 5, 3, 1, p, p, p), -1, b"NULL"),
        ((p, p, 1, 5, 3, 1, None, p, p), -1, b"NULL"),
        ((p, p, 1, 5, 3, 1, p, None, p), -1, b"NULL"),
        ((p, p, 1, 5, 3, 1, p, p, None), -1, b"NULL"),
        ((p, p, 1, 5, 0, 1, p, p, p), -1, b"max_seg=0"),
        ((p, p, 1, 5, 4, 1, p, p, p), -1, b"max_seg=4"),
        ((p, p, 0, 5, 3, 1, p, p, p), -1, b"B=0"),
        ((p, p, 1, 2, 3, 1, p, p, p), -1, b"n=2"),
        ((p, p, 1, 1025, 3, 1, p, p, p), -3, b"n=1025"),
    ]
    for args, code, msg in scan:
        assert lib.gnngls_or_opt_best_move(*args, None) == code, args
        err = lib.gnngls_last_error()
        assert b"or_opt_best_move" in err and msg in err, (args, err)
    # tour, cost, D, B, n, max_seg, reverse, max_moves, tour_out, cost_out, moves, status, trace_cost, trace_cap
    ok = [p, p, p, 1, 5, 3, 1, 10, p, p, p, p, None, 0]
    descent = [({k: None}, -1, b"NULL") for k in (0, 1, 2, 8, 9, 10, 11)]
    descent += [({5: 0}, -1, b"max_seg=0"), ({5: 4}, -1, b"max_seg=4"), ({7: 0}, -1, b"max_moves=0"), ({7: -3}, -1, b"max_moves=-3"),
                ({13: -1}, -1, b"trace_cap=-1"), ({3: 0}, -1, b"B=0"), ({4: 2}, -1, b"n=2"), ({4: 1025}, -3, b"n=1025")]
    for change, code, msg in descent:
        args = list(ok)
        for k, v in change.items():
            args[k] = v
        assert lib.gnngls_or_opt_descent(*args, None) == code, args
        err = lib.gnngls_last_error()
        assert b"or_opt_descent" in err and msg in err, (args, err)


def test_torch_op_has_a_shape_function_and_no_cpu_kernel():
    import torch
    import gnngls_amd.torch_ops  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        t = torch.empty((5, 10), dtype=torch.int32, device="cuda")
        c = torch.empty((5,), dtype=torch.float64, device="cuda")
        D = torch.empty((5, 9, 9), dtype=torch.float64, device="cuda")
        tour, cost, moves, status, trace = torch.ops.gnngls.or_opt_descent(t, c, D, 3, True, 900, 7)
        assert tour.shape == (5, 10) and tour.dtype == torch.int32 and cost.shape == (5,) and cost.dtype == torch.float64
        assert moves.shape == status.shape == (5,) and moves.dtype == status.dtype == torch.int32
        assert trace.shape == (5, 7) and trace.dtype == torch.float64
    with pytest.raises(NotImplementedError):
        torch.ops.gnngls.or_opt_descent(torch.zeros((1, 5), dtype=torch.int32), torch.zeros(1, dtype=torch.float64),
                                        torch.zeros((1, 4, 4), dtype=torch.float64), 3, True, 10, 0)


def test_python_surface():
    from gnngls_amd import algorithms, operators, ops, pipeline
    sig = inspect.signature(pipeline.solve_batch)
    assert sig.parameters["polish"].default is None and sig.parameters["polish_seg"].default == 3
    assert "polish_gain" in {f.name for f in __import__("dataclasses").fields(pipeline.SolveResult)}
    assert list(inspect.signature(ops.or_opt_best_move).parameters) == ["tour", "D", "max_seg", "reverse"]
    assert list(inspect.signature(ops.or_opt_descent).parameters) == ["tour", "cost", "D", "max_seg", "reverse", "max_moves", "trace_cap"]
    assert list(inspect.signature(operators.or_opt_a2a).parameters) == ["tour", "D", "max_seg", "reverse"]
    assert list(inspect.signature(algorithms.or_opt_descent).parameters) == ["init_tour", "init_cost", "D", "max_seg", "reverse"]
    for f in (ops.or_opt_best_move, ops.or_opt_descent, operators.or_opt_a2a, algorithms.or_opt_descent, host.or_opt_a2a, host.or_opt_descent):
        p = inspect.signature(f).parameters
        assert p["max_seg"].default == 3 and p["reverse"].default is True, f
    assert ops.OR_OPT_MAX_N == 1024 and ops.STATUS_MOVE_CAP == 6
    with pytest.raises(ValueError, match="unknown polish"):
        pipeline.solve_batch(None, polish="three_opt")
    # the host-side mirrors of a move agree with the definition
    tour = [0, 3, 1, 4, 2, 5, 0]
    assert operators.or_opt(tour, 2, 2, 1, 3) == host.or_opt(tour, 2, 2, 1, 3) == [0, 3, 2, 4, 1, 5, 0]
    D = euclid(np.random.default_rng(6), 6)
    assert bits(operators.or_opt_cost(tour, D, 2, 2, 1, 3)) == bits(host.or_opt_cost(tour, D, 2, 2, 1, 3))


def test_cli_names_the_flags():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "test.py"), "--help"], capture_output=True, text=True, cwd=ROOT)
    assert out.returncode == 0 and "--polish" in out.stdout and "--polish_seg" in out.stdout
