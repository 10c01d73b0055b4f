"""CPU checks of 3-opt (gnngls_three_opt_best_move, gnngls_three_opt_descent; the definition in include/gnngls_hip.h): the NumPy
restatement in gnngls_amd.host -- the reference of the GPU tests -- agrees with brute force, contains every Or-opt candidate, keeps
the stated tie rule and ends in local optima; and the boundary is in place: the entries are exported with ctypes signatures,
argument errors are answered on the host before any HIP call, the torch operator has a shape function.  The kernels' arithmetic is
pinned on the GPU (tests/test_three_opt_gpu.py).  Equality means equal bit patterns for every fp64 value and equal tours."""
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from gnngls_amd import host  # noqa: E402
from test_alpha_cpu import tie_heavy  # noqa: E402
from test_one_tree_cpu import euclid  # noqa: E402
from test_or_opt_cpu import bits, nn_tour, random_tour, tour_cost  # noqa: E402
from test_or_opt_cpu import candidates as or_opt_candidates  # noqa: E402


def candidates(n):
    """Every (p1, p2, p3, kind) of the definition, in its enumeration order."""
    for p1 in range(0, n - 2):
        for p2 in range(p1 + 1, n - 1):
            for p3 in range(p2 + 1, n):
                for kind in range(4):
                    yield p1, p2, p3, kind


def literal_a2a(tour, D):
    """The scan as the definition words it: a four-deep loop in the stated order under the reference's acceptance rule."""
    best_delta, best_move = 0, None
    for p1, p2, p3, kind in candidates(len(tour) - 1):
        delta = host.three_opt_cost(tour, D, p1, p2, p3, kind)
        if delta < best_delta and not np.isclose(0, delta):
            best_delta, best_move = delta, (p1, p2, p3, kind)
    return best_delta, best_move


def test_candidate_count():
    for n in (3, 4, 7, 10):
        assert len(list(candidates(n))) == 4 * n * (n - 1) * (n - 2) // 6
    assert list(candidates(3)) == [(0, 1, 2, k) for k in range(4)]


@pytest.mark.parametrize("n", range(4, 11))
def test_definition_against_brute_force(n):
    rng = np.random.default_rng(300 + n)
    D = euclid(rng, n)
    for _ in range(3):
        tour = random_tour(rng, n)
        old = tour_cost(tour, D)
        for p1, p2, p3, kind in candidates(n):
            new = host.three_opt(tour, p1, p2, p3, kind)
            assert len(new) == n + 1 and new[0] == new[-1] == 0 and sorted(new[:-1]) == list(range(n)), (tour, p1, p2, p3, kind)
            assert new[:p1 + 1] == tour[:p1 + 1] and new[p3 + 1:] == tour[p3 + 1:]          # head and tail stay
            delta = host.three_opt_cost(tour, D, p1, p2, p3, kind)
            assert abs(delta - (tour_cost(new, D) - old)) <= 1e-9, (tour, p1, p2, p3, kind, delta)
        want = literal_a2a(tour, D)
        got = host.three_opt_a2a(tour, D)
        assert got[1] == want[1] and bits(got[0]) == bits(want[0]), (n, got, want)


def test_the_four_reconnections_by_hand():
    tour = [0, 1, 2, 3, 4, 5, 6, 0]                    # H = 0 1 | B = 2 3 | C = 4 5 | T = 6 0
    assert host.three_opt(tour, 1, 3, 5, 0) == [0, 1, 3, 2, 5, 4, 6, 0]
    assert host.three_opt(tour, 1, 3, 5, 1) == [0, 1, 4, 5, 2, 3, 6, 0]
    assert host.three_opt(tour, 1, 3, 5, 2) == [0, 1, 5, 4, 2, 3, 6, 0]
    assert host.three_opt(tour, 1, 3, 5, 3) == [0, 1, 4, 5, 3, 2, 6, 0]
    # the operand order of the delta: kind 2 adds D[a1,c2], D[c1,b1], D[b2,a2] and removes D[a1,b1], D[b2,c1], D[c2,a2]
    D = euclid(np.random.default_rng(7), 7)
    want = ((((D[1, 5] + D[4, 2]) + D[3, 6]) - D[1, 2]) - D[3, 4]) - D[5, 6]
    assert bits(host.three_opt_cost(tour, D, 1, 3, 5, 2)) == bits(want)


@pytest.mark.parametrize("n", range(5, 11))
def test_every_or_opt_candidate_is_a_three_opt_move(n):
    rng = np.random.default_rng(500 + n)
    tour = random_tour(rng, n)
    pure = {tuple(host.three_opt(tour, *c)) for c in candidates(n)}
    misses = [c for c in or_opt_candidates(n, 3, True) if tuple(host.or_opt(tour, *c)) not in pure]
    assert not misses, misses[:5]


@pytest.mark.parametrize("n", [8, 20, 64])
def test_tie_rule_equals_the_literal_loop(n):
    rng = np.random.default_rng(n)
    D = tie_heavy(rng, n)
    for tour in (nn_tour(D), random_tour(rng, n)):
        want = literal_a2a(tour, D)
        got = host.three_opt_a2a(tour, D)
        assert got[1] == want[1] and bits(got[0]) == bits(want[0]), (n, got, want)
    if n == 20:                                         # from the nearest-neighbour tour six candidates tie at the minimum
        tour = nn_tour(D)
        deltas = [host.three_opt_cost(tour, D, *c) for c in candidates(n)]
        assert min(deltas) == -2.0 and sum(d == -2.0 for d in deltas) == 6
        assert host.three_opt_a2a(tour, D) == (-2.0, (0, 2, 13, 0))


@pytest.mark.parametrize("n", [3, 5, 20, 64])
def test_descent_ends_in_a_local_optimum_of_both_scans(n):
    for D in (euclid(np.random.default_rng(1000 + n), n), tie_heavy(np.random.default_rng(2000 + n), n)):
        init = nn_tour(D)
        c0 = tour_cost(init, D)
        tour, cost, moves, trace = host.three_opt_descent(init, c0, D)
        assert host.two_opt_a2a(tour, D) == (0, None) and host.three_opt_a2a(tour, D) == (0, None)
        assert moves == len(trace) and sorted(tour[:-1]) == list(range(n)) and tour[0] == tour[-1] == 0
        assert abs(cost - tour_cost(tour, D)) <= 1e-9 * max(cost, 1) and all(b < a for a, b in zip([c0] + trace, trace))
        if n == 3:
            assert moves == 0 and tour == init
        # the cap is checked after every move: the first k moves of the same trajectory
        for k in range(1, min(moves, 3) + 1):
            t2, c2, m2, tr2 = host.three_opt_descent(init, c0, D, max_moves=k)
            assert m2 == k and np.array_equal(bits(tr2), bits(trace[:k])) and bits(c2) == bits(trace[k - 1])


@pytest.fixture(scope="module")
def lib():
    from gnngls_amd import _lib, build
    build.build()
    return _lib.load()


def test_entries_exported_with_signatures(lib):
    from gnngls_amd import _lib
    raw = ctypes.CDLL(_lib.SO)
    for name, nargs in (("gnngls_three_opt_best_move", 8), ("gnngls_three_opt_descent", 13), ("gnngls_three_opt_lds_max_n", 0)):
        assert hasattr(raw, name) and name in _lib.SIGNATURES
        assert len(getattr(lib, name).argtypes) == nargs
    assert lib.gnngls_abi_version() == 4
    assert 0 <= lib.gnngls_three_opt_lds_max_n() <= 256
    h = open(os.path.join(ROOT, "include", "gnngls_hip.h")).read()
    for word in ("gnngls_three_opt_best_move(", "gnngls_three_opt_descent(", "GNNGLS_THREE_OPT_MAX_N 256", "(p1, p2, p3, kind)",
                 "delta = ((((x + y) + z) - D[a1,b1]) - D[b2,c1]) - D[c2,a2]", "D[a1,c2], D[c1,b1], D[b2,a2]"):
        assert word in h, word


def test_argument_checks_answer_before_any_device_work(lib):
    """No GPU here: an entry that reached a HIP call would answer GNNGLS_ERR_HIP (-2), not these codes."""
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    # tour, D, B, n, delta, move, new_tour
    ok = [p, p, 1, 5, p, p, p]
    scan = [({k: None}, -1, b"NULL") for k in (0, 1, 4, 5, 6)]
    scan += [({2: 0}, -1, b"B=0"), ({2: -4}, -1, b"B=-4"), ({3: 2}, -1, b"n=2"), ({3: 257}, -3, b"n=257")]
    for change, code, msg in scan:
        args = list(ok)
        for k, v in change.items():
            args[k] = v
        assert lib.gnngls_three_opt_best_move(*args, None) == code, args
        err = lib.gnngls_last_error()
        assert b"three_opt_best_move" in err and msg in err, (args, err)
    # tour, cost, D, B, n, max_moves, tour_out, cost_out, moves, status, trace_cost, trace_cap
    ok = [p, p, p, 1, 5, 10, p, p, p, p, None, 0]
    descent = [({k: None}, -1, b"NULL") for k in (0, 1, 2, 6, 7, 8, 9)]
    descent += [({5: 0}, -1, b"max_moves=0"), ({5: -3}, -1, b"max_moves=-3"), ({11: -1}, -1, b"trace_cap=-1"),
                ({11: 4}, -1, b"trace_cap=4"),                                   # a NULL trace_cost only with trace_cap 0
                ({3: 0}, -1, b"B=0"), ({4: 2}, -1, b"n=2"), ({4: 257}, -3, b"n=257")]
    for change, code, msg in descent:
        args = list(ok)
        for k, v in change.items():
            args[k] = v
        assert lib.gnngls_three_opt_descent(*args, None) == code, args
        err = lib.gnngls_last_error()
        assert b"three_opt_descent" in err and msg in err, (args, err)


def test_torch_op_has_a_shape_function_and_no_cpu_kernel():
    import torch
    import gnngls_amd.torch_ops  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        t = torch.empty((5, 10), dtype=torch.int32, device="cuda")
        c = torch.empty((5,), dtype=torch.float64, device="cuda")
        D = torch.empty((5, 9, 9), dtype=torch.float64, device="cuda")
        tour, cost, moves, status, trace = torch.ops.gnngls.three_opt_descent(t, c, D, 900, 7)
        assert tour.shape == (5, 10) and tour.dtype == torch.int32 and cost.shape == (5,) and cost.dtype == torch.float64
        assert moves.shape == status.shape == (5,) and moves.dtype == status.dtype == torch.int32
        assert trace.shape == (5, 7) and trace.dtype == torch.float64
    with pytest.raises(NotImplementedError):
        torch.ops.gnngls.three_opt_descent(torch.zeros((1, 5), dtype=torch.int32), torch.zeros(1, dtype=torch.float64),
                                           torch.zeros((1, 4, 4), dtype=torch.float64), 10, 0)


def test_python_surface():
    from gnngls_amd import algorithms, operators, ops
    assert list(inspect.signature(ops.three_opt_best_move).parameters) == ["tour", "D"]
    assert list(inspect.signature(ops.three_opt_launch).parameters) == ["tour", "cost", "D", "max_moves", "trace_cap"]
    assert list(inspect.signature(ops.three_opt_descent).parameters) == ["tour", "cost", "D", "max_moves", "trace_cap"]
    assert list(inspect.signature(host.three_opt_cost).parameters) == ["tour", "D", "p1", "p2", "p3", "kind"]
    assert list(inspect.signature(host.three_opt).parameters) == ["tour", "p1", "p2", "p3", "kind"]
    assert list(inspect.signature(host.three_opt_a2a).parameters) == ["tour", "D"]
    assert list(inspect.signature(host.three_opt_descent).parameters) == ["tour", "cost", "D", "max_moves"]
    assert list(inspect.signature(operators.three_opt).parameters) == ["tour", "p1", "p2", "p3", "kind"]
    assert list(inspect.signature(operators.three_opt_cost).parameters) == ["tour", "D", "p1", "p2", "p3", "kind"]
    assert list(inspect.signature(operators.three_opt_a2a).parameters) == ["tour", "D"]
    assert list(inspect.signature(algorithms.three_opt_descent).parameters) == ["init_tour", "init_cost", "D"]
    p = inspect.signature(ops.three_opt_descent).parameters
    assert p["max_moves"].default is None and p["trace_cap"].default == 0
    assert ops.THREE_OPT_MAX_N == 256
    assert {f.name for f in __import__("dataclasses").fields(ops.ThreeOptResult)} == \
        {f.name for f in __import__("dataclasses").fields(ops.OrOptResult)}
    # the host-side mirrors of a move agree with the definition
    tour = [0, 3, 1, 4, 2, 5, 0]
    D = euclid(np.random.default_rng(6), 6)
    for c in candidates(6):
        assert operators.three_opt(tour, *c) == host.three_opt(tour, *c)
        assert bits(operators.three_opt_cost(tour, D, *c)) == bits(host.three_opt_cost(tour, D, *c))


def test_bench_script_names_its_flags():
    import subprocess
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "bench_three_opt.py"), "--help"], capture_output=True, text=True,
                         cwd=ROOT)
    assert out.returncode == 0 and "--shapes" in out.stdout and "--after_shapes" in out.stdout and "--out" in out.stdout
