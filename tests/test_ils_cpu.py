"""CPU checks of iterated local search (gnngls_ils_run; the definition in include/gnngls_hip.h): the NumPy restatement in
gnngls_amd.host -- the reference of the GPU tests -- draws every cut-point triple and only those, kicks with a true double bridge
whose delta is the difference of the two tour costs, runs as a prefix-stable loop that chains with kick0, and does improve on the
descent alone; its Philox is the Random123 generator of the sampled walks.  And the boundary is in place: the entry is exported
with a ctypes signature, argument errors are answered on the host before any HIP call, the torch operator has a shape function.
The kernel's arithmetic is pinned on the GPU (tests/test_ils_gpu.py).  Equality means equal bit patterns and equal tours."""
import ctypes
import inspect
import itertools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from gnngls_amd import host  # noqa: E402
from test_one_tree_cpu import euclid  # noqa: E402
from test_or_opt_cpu import bits, nn_tour, random_tour, tour_cost  # noqa: E402
import test_sampling_cpu as sampling  # noqa: E402

U_MAX = 1.0 - 2.0 ** -53


def triples(n):
    return set(itertools.combinations(range(1, n), 3))


def undirected(tour):
    return {frozenset(e) for e in zip(tour[:-1], tour[1:])}


@pytest.mark.parametrize("n,count", [(4, 1), (5, 4), (6, 10), (9, 56)])
def test_cuts_reach_exactly_the_triples(n, count):
    grid = (np.arange(64) + 0.5) / 64
    seen = {host.double_bridge_cuts((a, b, c), n) for a in grid for b in grid for c in grid}
    assert seen == triples(n) and len(seen) == count


@pytest.mark.parametrize("n", [4, 5, 6, 9, 40, 1024])
def test_cuts_stay_in_range_at_the_ends_of_the_unit_interval(n):
    for u in itertools.product((0.0, U_MAX), repeat=3):
        p1, p2, p3 = host.double_bridge_cuts(u, n)
        assert 1 <= p1 < p2 < p3 <= n - 1, (n, u)
    assert host.double_bridge_cuts((0.0, 0.0, 0.0), n) == (1, 2, 3)
    assert host.double_bridge_cuts((U_MAX,) * 3, n) == (n - 3, n - 2, n - 1)


def check_kick(tour, D, p1, p2, p3):
    n = len(tour) - 1
    new = host.double_bridge(tour, p1, p2, p3)
    assert len(new) == n + 1 and new[0] == new[-1] == tour[0] and sorted(new[:-1]) == list(range(n)), (tour, p1, p2, p3)
    assert new == tour[:p1] + tour[p3:n] + tour[p2:p3] + tour[p1:p2] + [tour[n]]
    changed = len(undirected(tour) - undirected(new))
    assert changed <= 4
    if p2 - p1 >= 2 and p3 - p2 >= 2:
        # A D C B: a true double bridge, no segment swap.  One corner has three: A = [depot] and Dseg one node d, where the new
        # junction (depot, d) is the old closing edge (d, depot) read the other way
        assert changed == (3 if p1 == 1 and p3 == n - 1 else 4), (tour, p1, p2, p3)
    old = tour_cost(tour, D)
    delta = host.double_bridge_cost(tour, D, p1, p2, p3)
    assert abs(delta - (tour_cost(new, D) - old)) <= 1e-12 * old, (tour, p1, p2, p3, delta)


def test_kick_is_a_double_bridge_and_its_delta_the_cost_difference():
    rng = np.random.default_rng(9)
    D = euclid(rng, 9)
    tour = random_tour(rng, 9)
    for p in sorted(triples(9)):
        check_kick(tour, D, *p)
    D = euclid(rng, 40)
    for _ in range(60):
        p = sorted(rng.choice(np.arange(1, 40), 3, replace=False).tolist())
        check_kick(random_tour(rng, 40), D, *p)
    # the operand order of the definition
    t = [0, 1, 2, 3, 4, 5, 0]
    D = euclid(rng, 6)
    want = D[1, 5] + D[5, 4] + D[4, 2] + D[3, 0] - D[1, 2] - D[3, 4] - D[4, 5] - D[5, 0]
    assert bits(host.double_bridge_cost(t, D, 2, 4, 5)) == bits(want)
    assert host.double_bridge(t, 2, 4, 5) == [0, 1, 5, 4, 2, 3, 0]


def instance(n, seed):
    D = euclid(np.random.default_rng(seed), n)
    init = nn_tour(D)
    return D, init, tour_cost(init, D)


def same(a, b):
    return a[0] == b[0] and bits(a[1]) == bits(b[1]) and a[2:5] == b[2:5] and np.array_equal(bits(a[5]), bits(b[5]))


@pytest.mark.parametrize("n", [5, 12, 30])
def test_run_is_prefix_stable_and_chains(n):
    D, init, c0 = instance(n, 5000 + n)
    K = 6
    u = np.random.default_rng(n).random((2 * K, 3))
    zero = host.ils(init, c0, D, 0)
    dt, dc, dm, _ = host.or_opt_descent(init, c0, D)
    assert zero == (dt, dc, dm, 0, 0, [])
    short = host.ils(init, c0, D, K, u=u[:K])
    full = host.ils(init, c0, D, 2 * K, u=u)
    assert np.array_equal(bits(full[5][:K]), bits(short[5])) and len(full[5]) == 2 * K
    assert full[1] <= short[1] <= dc and full[3] >= short[3] and full[2] >= short[2]
    # the accumulated cost is the tour's cost
    for r in (short, full):
        assert sorted(r[0][:-1]) == list(range(n)) and r[0][0] == r[0][-1] == 0
        assert abs(r[1] - tour_cost(r[0], D)) <= 1e-9 * r[1]
        assert r[4] == 0
    # K1 kicks, then K2 more from the outputs: the second run's first descent applies nothing
    rest = host.ils(short[0], short[1], D, K, u=u[K:])
    assert rest[0] == full[0] and bits(rest[1]) == bits(full[1]) and short[2] + rest[2] == full[2]
    assert short[3] + rest[3] == full[3] and np.array_equal(bits(short[5] + rest[5]), bits(full[5]))
    # and the same through the generator: kick0 offsets the counter
    a = host.ils(init, c0, D, 4, seed=77, b=3)
    b2 = host.ils(a[0], a[1], D, 5, seed=77, b=3, kick0=4)
    whole = host.ils(init, c0, D, 9, seed=77, b=3)
    assert b2[0] == whole[0] and bits(b2[1]) == bits(whole[1]) and np.array_equal(bits(a[5] + b2[5]), bits(whole[5]))
    assert same(whole, host.ils(init, c0, D, 9, u=host.philox_uniforms(77, 1, 9, 3, b0=3, c3=1)[0]))
    # accepted kicks are the strict improvements of the running cost
    cur, acc = dc, 0
    for c in whole[5]:
        if c - cur < 0 and not np.isclose(0, c - cur):
            cur, acc = c, acc + 1
    assert acc == whole[3] and bits(cur) == bits(whole[1])


def test_move_cap_ends_the_run():
    D, init, c0 = instance(30, 5030)
    u = np.random.default_rng(1).random((8, 3))
    free = host.ils(init, c0, D, 8, u=u)
    first = host.or_opt_descent(init, c0, D)[2]
    assert free[2] > first + 3
    for cap in (1, first, first + 1, first + 3, free[2] - 1):
        r = host.ils(init, c0, D, 8, max_moves=cap, u=u)
        assert r[2] == cap and r[4] == host.ILS_STATUS_MOVE_CAP, (cap, r[2:5])
        done = max(len(r[5]) - 1, 0)                            # kicks whose descent the cap did not cut short
        assert np.array_equal(bits(r[5][:done]), bits(free[5][:done])) and len(r[5]) <= 8
        assert abs(r[1] - tour_cost(r[0], D)) <= 1e-9 * r[1]
        assert len(r[5]) == 0 if cap <= first else len(r[5]) >= 1
    # a cap the run never reaches changes nothing; one it reaches with its last move still reports it
    assert same(host.ils(init, c0, D, 8, max_moves=free[2] + 1, u=u), free)
    assert host.ils(init, c0, D, 8, max_moves=free[2], u=u)[4] == host.ILS_STATUS_MOVE_CAP


def test_kicks_improve_on_the_descent_alone():
    """The quality condition, on the definition alone: of 8 uniform instances at n = 60, 30 kicks must take at least one more than
    1e-7 (relative) below its descent-only cost (this generator and these seeds: 8 of 8)."""
    better = 0
    for s in range(8):
        D, init, c0 = instance(60, 6000 + s)
        base = host.or_opt_descent(init, c0, D)[1]
        r = host.ils(init, c0, D, 30, seed=s)
        assert r[1] <= base
        better += r[1] < base * (1 - 1e-7)
    assert better >= 1, better


def test_philox_is_the_generator_of_the_sampled_walks():
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, out in kat:
        assert tuple(int(x) for x in host.philox4x32_10(*ctr, *key)) == out
        assert tuple(int(x) for x in sampling.philox4x32_10(*ctr, *key)) == out
    seed = 0x123456789abcdef
    assert np.array_equal(bits(host.philox_uniforms(seed, 3, 4, 9)), bits(sampling.philox_uniforms(seed, 3, 4, 9)))
    assert np.array_equal(bits(host.philox_uniforms(seed, 1, 2, 9, b0=2, k0=1)), bits(sampling.philox_uniforms(seed, 1, 2, 9, b0=2, r0=1)))
    u1 = host.philox_uniforms(seed, 3, 4, 3, c3=1)
    assert u1.shape == (3, 4, 3) and (u1 >= 0).all() and (u1 < 1).all()
    assert not np.intersect1d(u1, host.philox_uniforms(seed, 3, 4, 3)).size          # the two streams are apart
    o = host.philox4x32_10(2, 3, 1, 1, seed & 0xFFFFFFFF, seed >> 32)
    assert bits(u1[2, 3, 1]) == bits(float(((int(o[0]) << 32) | int(o[1])) >> 11) * 2.0 ** -53)


@pytest.fixture(scope="module")
def lib():
    from gnngls_amd import _lib, build
    build.build()
    return _lib.load()


def test_entry_exported_with_signature(lib):
    from gnngls_amd import _lib
    raw = ctypes.CDLL(_lib.SO)
    assert hasattr(raw, "gnngls_ils_run") and "gnngls_ils_run" in _lib.SIGNATURES and "gnngls_ils_run" in _lib._ILS
    assert len(lib.gnngls_ils_run.argtypes) == 19 and lib.gnngls_ils_run.argtypes[10] is ctypes.c_uint64
    assert lib.gnngls_abi_version() == 4


def test_argument_checks_answer_before_any_device_work(lib):
    """No GPU here: an entry that reached a HIP call would answer GNNGLS_ERR_HIP (-2), not these codes."""
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    # tour, cost, D, B, n, kicks, kick0, max_seg, reverse, max_moves, seed, u, tour_out, cost_out, moves, accepted, status, trace
    ok = [p, p, p, 1, 5, 3, 0, 3, 1, 10, 7, None, p, p, p, p, p, None]
    cases = [({k: None}, -1, b"NULL") for k in (0, 1, 2, 12, 13, 14, 15, 16)]
    cases += [({4: 3}, -1, b"n=3"), ({4: 0}, -1, b"n=0"), ({4: 1025}, -3, b"n=1025"), ({3: 0}, -1, b"B=0"), ({3: -2}, -1, b"B=-2"),
              ({5: -1}, -1, b"kicks=-1"), ({6: -1}, -1, b"kick0=-1"), ({5: 2 ** 31 - 1, 6: 1}, -1, b"kick0 + kicks"),
              ({5: 1, 6: 2 ** 31 - 1}, -1, b"kick0 + kicks"), ({7: 0}, -1, b"max_seg=0"), ({7: 4}, -1, b"max_seg=4"),
              ({9: 0}, -1, b"max_moves=0"), ({9: -5}, -1, b"max_moves=-5")]
    for change, code, msg in cases:
        args = list(ok)
        for k, v in change.items():
            args[k] = v
        assert lib.gnngls_ils_run(*args, None) == code, args
        err = lib.gnngls_last_error()
        assert b"ils_run" in err and msg in err, (args, err)


def test_torch_op_has_a_shape_function_and_no_cpu_kernel():
    import torch
    import gnngls_amd.torch_ops  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        t = torch.empty((5, 10), dtype=torch.int32, device="cuda")
        c = torch.empty((5,), dtype=torch.float64, device="cuda")
        D = torch.empty((5, 9, 9), dtype=torch.float64, device="cuda")
        tour, cost, moves, accepted, status, trace = torch.ops.gnngls.ils(t, c, D, 7, 0, 3, True, 900, 1, None)
        assert tour.shape == (5, 10) and tour.dtype == torch.int32 and cost.shape == (5,) and cost.dtype == torch.float64
        assert moves.shape == accepted.shape == status.shape == (5,) and moves.dtype == accepted.dtype == status.dtype == torch.int32
        assert trace.shape == (5, 7) and trace.dtype == torch.float64
    with pytest.raises(NotImplementedError):
        torch.ops.gnngls.ils(torch.zeros((1, 6), dtype=torch.int32), torch.zeros(1, dtype=torch.float64),
                             torch.zeros((1, 5, 5), dtype=torch.float64), 2, 0, 3, True, 10, 0, None)


def test_python_surface():
    import dataclasses
    from gnngls_amd import algorithms, ops
    assert list(inspect.signature(host.ils).parameters) == ["tour", "cost", "D", "kicks", "max_seg", "reverse", "max_moves", "u", "seed",
                                                            "b", "kick0"]
    assert list(inspect.signature(ops.ils).parameters) == ["tour", "cost", "D", "kicks", "max_seg", "reverse", "max_moves", "seed", "u",
                                                           "kick0", "want_trace"]
    assert list(inspect.signature(ops.ils_launch).parameters) == list(inspect.signature(ops.ils).parameters)
    assert list(inspect.signature(algorithms.iterated_local_search).parameters) == ["init_tour", "init_cost", "D", "kicks", "max_seg",
                                                                                    "reverse", "seed"]
    for f in (host.ils, ops.ils, ops.ils_launch, algorithms.iterated_local_search):
        p = inspect.signature(f).parameters
        assert p["max_seg"].default == 3 and p["reverse"].default is True, f
    assert inspect.signature(algorithms.iterated_local_search).parameters["seed"].default is None
    assert [f.name for f in dataclasses.fields(ops.IlsResult)] == ["tour", "cost", "moves", "accepted", "status", "trace_cost"]
    assert host.ILS_STATUS_MOVE_CAP == ops.STATUS_MOVE_CAP == 6


def test_header_and_docs_carry_the_contract():
    h = open(os.path.join(ROOT, "include", "gnngls_hip.h")).read()
    for word in ("gnngls_ils_run(", "p1 = 1 + min(int(u0 * (m - 2)), m - 3)", "p2 = p1 + 1 + min(int(u1 * (m - 1 - p1)), m - 2 - p1)",
                 "p3 = p2 + 1 + min(int(u2 * (m - p2)), m - 1 - p2)", "A + Dseg + C + B + [t[n]]",
                 "D[ae,ds] + D[de,cs] + D[ce,bs] + D[be,z] - D[ae,bs] - D[be,cs] - D[ce,ds] - D[de,z]",
                 "not np.isclose(0, d)", "(b, kick0 + k, s, 1)", "GNNGLS_STATUS_MOVE_CAP", "kicks = 0 is exactly gnngls_or_opt_descent"):
        assert word in h, word
    doc = inspect.getdoc(host.ils)
    for word in ("double_bridge_cuts", "not np.isclose(0, d)", "kick0"):
        assert word in doc, word
    for name, words in (("README.md", ("ils_kernel", "bench_ils.py", "profiles/ils.json")), ("DESIGN.md", ("ils_kernel", "double bridge")),
                        ("INTEGRATION.md", ("ops.ils(", "torch.ops.gnngls.ils", "iterated_local_search", "gnngls_ils_run"))):
        text = open(os.path.join(ROOT, name)).read()
        for word in words:
            assert word in text, (name, word)
