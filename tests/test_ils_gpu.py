"""GPU checks of iterated local search (gnngls_ils_run; ils_kernel in oropt_kernels.hip) against the NumPy restatement of its
definition in gnngls_amd.host (itself pinned in tests/test_ils_cpu.py): equality always means equal bit patterns of every fp64
value and equal tours.  Instances are euclid(default_rng(1000 + n), n) from the nearest-neighbour start, as in the Or-opt tests."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from gnngls_amd import host  # noqa: E402
from test_alpha_cpu import tie_heavy  # noqa: E402
from test_one_tree_cpu import euclid  # noqa: E402
from test_or_opt_cpu import bits  # noqa: E402

# the single triple (4), a handful (5, 6, 9), two and three wavefronts (17, 33), the lane loop's edge (64, 65), 100, and the
# two-step arg-min (129: nine wavefronts)
SIZES = (4, 5, 6, 9, 17, 33, 64, 65, 100, 129)
SETTINGS = [(1, False), (3, True)]
U_MAX = 1.0 - 2.0 ** -53
SENTINEL = -12345.0


def dev(x, dtype=torch.float64):
    from gnngls_amd import ops
    return ops.as_dev(np.asarray(x), dtype)


def same_bits(a, b):
    """torch.equal on the bit patterns (fp64 tensors may hold NaN)."""
    return torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a, b.view(torch.int64) if b.dtype == torch.float64 else b)


_cache = {}


def load(n, count=None):
    """-> (Ds [count,n,n], D on the device, nearest-neighbour tours on the device, their costs, the tours as lists, the costs as
    floats); built once per size."""
    from gnngls_amd import ops
    count = count or (3 if n <= 33 else 2)
    if (n, count) not in _cache:
        rng = np.random.default_rng(1000 + n)
        Ds = np.stack([euclid(rng, n) for _ in range(count)])
        D = dev(Ds)
        t = ops.nearest_neighbor(D)
        c = ops.tour_cost(t, D)
        _cache[n, count] = (Ds, D, t, c, t.cpu().numpy().tolist(), c.cpu().numpy())
    return _cache[n, count]


def kicks_for(n):
    return 12 if n <= 33 else 4


def assert_ils(r, tours, costs, Ds, kicks, max_seg, reverse, what, u=None, seed=0, kick0=0, max_moves=None, b0=0):
    """Every output of the launch against host.ils per instance; trace entries of kicks that never ran must be NaN (as given)."""
    tour, cost, moves, acc, st = (x.cpu().numpy() for x in (r.tour, r.cost, r.moves, r.accepted, r.status))
    trace = r.trace_cost.cpu().numpy()
    want = []
    for b, D in enumerate(Ds):
        w = host.ils(tours[b], costs[b], D, kicks, max_seg, reverse, max_moves, None if u is None else u[b], seed, b0 + b, kick0)
        assert tour[b].tolist() == w[0], (what, b)
        assert bits(cost[b]) == bits(w[1]), (what, b, cost[b], w[1])
        assert (int(moves[b]), int(acc[b]), int(st[b])) == w[2:5], (what, b, moves[b], acc[b], st[b], w[2:5])
        ran = len(w[5])
        assert np.array_equal(bits(trace[b, :ran]), bits(w[5])), (what, b)
        assert np.isnan(trace[b, ran:]).all(), (what, b)
        want.append(w)
    return want


@pytest.mark.parametrize("n", SIZES)
def test_run_equals_the_host_definition(n):
    from gnngls_amd import ops
    Ds, D, t, c, tours, costs = load(n)
    K = kicks_for(n)
    u = np.random.default_rng(2000 + n).random((len(Ds), K, 3))
    accepted = 0
    for max_seg, reverse in SETTINGS:
        r = ops.ils(t, c, D, K, max_seg, reverse, u=dev(u), want_trace=True)
        want = assert_ils(r, tours, costs, Ds, K, max_seg, reverse, f"n={n} max_seg={max_seg} reverse={reverse}", u=u)
        accepted += sum(w[3] for w in want)
    assert accepted > 0 or n <= 9                              # by the host definition kicks are accepted at these sizes
    # without a trace buffer: the same result
    r0 = ops.ils(t, c, D, K, max_seg, reverse, u=dev(u))
    assert r0.trace_cost is None and all(torch.equal(getattr(r0, f), getattr(r, f)) for f in ("tour", "cost", "moves", "accepted", "status"))


@pytest.mark.parametrize("n", [4, 5, 9, 33, 65])
def test_uniforms_at_the_extremes(n):
    from gnngls_amd import ops
    Ds, D, t, c, tours, costs = load(n)
    K, B = 4, len(Ds)
    rows = {"zeros": np.zeros((B, K, 3)), "ones": np.full((B, K, 3), U_MAX),
            # pieces of one node: B = t[1:2], C = t[2:3] (0, 0, .); Dseg = t[n-1:n] (., ., max); A = [depot] throughout
            "single": np.tile(np.array([[0.0, 0.0, 0.0], [0.0, 0.0, U_MAX], [0.0, U_MAX, U_MAX], [U_MAX, 0.0, 0.0]]), (B, 1, 1))}
    for name, u in rows.items():
        r = ops.ils(t, c, D, K, 3, True, u=dev(u), want_trace=True)
        assert_ils(r, tours, costs, Ds, K, 3, True, f"n={n} u={name}", u=u)
    # values no generator gives still yield closed permutations (which: unspecified)
    wild = np.tile(np.array([[-1.0, 2.0, np.nan], [np.nan, -np.inf, 1e300], [1.0, 1.0, 1.0], [-0.0, np.inf, -1e-300]]), (B, 1, 1))
    r = ops.ils(t, c, D, K, 3, True, u=dev(wild))
    for b, row in enumerate(r.tour.cpu().numpy()):
        assert row[0] == row[-1] == 0 and sorted(row[:-1].tolist()) == list(range(n)), (n, b)
        assert abs(float(r.cost[b]) - sum(Ds[b][x, y] for x, y in zip(row[:-1], row[1:]))) <= 1e-9 * float(r.cost[b])


@pytest.mark.parametrize("n", [9, 33, 100])
def test_philox_path_equals_the_explicit_uniforms(n):
    from gnngls_amd import ops
    Ds, D, t, c, tours, costs = load(n)
    K, B, seed = kicks_for(n), len(Ds), 0x9e3779b97f4a7c15
    r = ops.ils(t, c, D, K, seed=seed, want_trace=True)
    u = host.philox_uniforms(seed, B, K, 3, c3=1)
    ru = ops.ils(t, c, D, K, u=dev(u), want_trace=True)
    for f in ("tour", "cost", "moves", "accepted", "status", "trace_cost"):
        assert same_bits(getattr(r, f), getattr(ru, f)), f
    assert_ils(r, tours, costs, Ds, K, 3, True, f"n={n} philox", seed=seed)
    # instance b of the batch is a B = 1 launch given that instance's uniforms
    for b in range(B):
        one = ops.ils(t[b:b + 1].contiguous(), c[b:b + 1].contiguous(), D[b:b + 1].contiguous(), K, u=dev(u[b:b + 1]), want_trace=True)
        assert torch.equal(one.tour[0], r.tour[b]) and bits(one.cost.cpu().numpy()[0]) == bits(r.cost.cpu().numpy()[b])
        assert np.array_equal(bits(one.trace_cost.cpu().numpy()[0]), bits(r.trace_cost.cpu().numpy()[b]))


@pytest.mark.parametrize("n", [4, 33, 100, 129])
def test_no_kicks_is_the_descent(n):
    from gnngls_amd import ops
    Ds, D, t, c, tours, costs = load(n)
    for max_seg, reverse in SETTINGS:
        r = ops.ils(t, c, D, 0, max_seg, reverse, want_trace=True)
        d = ops.or_opt_descent(t, c, D, max_seg, reverse)
        assert torch.equal(r.tour, d.tour) and torch.equal(r.cost.view(torch.int64), d.cost.view(torch.int64))
        assert torch.equal(r.moves, d.moves) and torch.equal(r.status, d.status) and not r.accepted.any()
        assert r.trace_cost.shape == (len(Ds), 0)


@pytest.mark.parametrize("n", [9, 33, 100])
def test_chained_runs_are_one_run(n):
    from gnngls_amd import ops
    Ds, D, t, c, tours, costs = load(n)
    K1, K2, seed = 3, kicks_for(n) - 3, 4242
    whole = ops.ils(t, c, D, K1 + K2, seed=seed, want_trace=True)
    a = ops.ils(t, c, D, K1, seed=seed, want_trace=True)
    b = ops.ils(a.tour, a.cost, D, K2, seed=seed, kick0=K1, want_trace=True)
    assert torch.equal(b.tour, whole.tour) and torch.equal(b.cost.view(torch.int64), whole.cost.view(torch.int64))
    assert torch.equal(a.moves + b.moves, whole.moves) and torch.equal(a.accepted + b.accepted, whole.accepted)
    assert torch.equal(torch.cat([a.trace_cost, b.trace_cost], 1).view(torch.int64), whole.trace_cost.view(torch.int64))
    assert_ils(b, a.tour.cpu().numpy().tolist(), a.cost.cpu().numpy(), Ds, K2, 3, True, f"n={n} kick0={K1}", seed=seed, kick0=K1)


@pytest.mark.parametrize("n", [12, 33])
def test_tie_heavy_instances(n):
    from gnngls_amd import ops
    rng = np.random.default_rng(4000 + n)
    Ds = np.stack([tie_heavy(rng, n) for _ in range(3)])
    D = dev(Ds)
    t = ops.nearest_neighbor(D)
    c = ops.tour_cost(t, D)
    u = rng.random((3, 12, 3))
    for max_seg, reverse in SETTINGS:
        r = ops.ils(t, c, D, 12, max_seg, reverse, u=dev(u), want_trace=True)
        assert_ils(r, t.cpu().numpy().tolist(), c.cpu().numpy(), Ds, 12, max_seg, reverse, f"ties n={n}", u=u)


def test_move_cap_ends_the_run_where_the_host_does():
    from gnngls_amd import ops
    Ds, D, t, c, tours, costs = load(33)
    K = 12
    u = np.random.default_rng(5).random((len(Ds), K, 3))
    free = ops.ils(t, c, D, K, u=dev(u)).moves.tolist()
    first = ops.or_opt_descent(t, c, D).moves.tolist()
    assert all(f > d + 4 for f, d in zip(free, first))
    for cap in (1, min(first), max(first) + 1, max(first) + 4, min(free) - 1, max(free), max(free) + 1):
        r = ops.ils(t, c, D, K, max_moves=cap, u=dev(u), want_trace=True)
        assert_ils(r, tours, costs, Ds, K, 3, True, f"max_moves={cap}", u=u, max_moves=cap)
        assert r.moves.tolist() == [min(cap, f) for f in free]
        assert r.status.tolist() == [ops.STATUS_MOVE_CAP if cap <= f else 0 for f in free]


def test_an_asymmetric_instance_is_reported_and_the_others_searched():
    from gnngls_amd import ops
    Ds, D, t, c, tours, costs = load(17, 4)
    bad = Ds.copy()
    bad[2, 3, 11] = np.nextafter(bad[2, 3, 11], 2.0)
    Db = dev(bad)
    K = 6
    u = np.random.default_rng(6).random((4, K, 3))
    r = ops.ils_launch(t, c, Db, K, u=dev(u), want_trace=True)
    assert r.status.tolist() == [0, 0, ops.STATUS_ASYMMETRIC, 0]
    assert torch.equal(r.tour[2], t[2]) and bits(r.cost.cpu().numpy()[2]) == bits(costs[2])
    assert int(r.moves[2]) == 0 and int(r.accepted[2]) == 0 and torch.isnan(r.trace_cost[2]).all()
    keep = [0, 1, 3]
    sub = ops.IlsResult(*(getattr(r, f)[keep] for f in ("tour", "cost", "moves", "accepted", "status", "trace_cost")))
    assert_ils(sub, [tours[b] for b in keep], costs[keep], Ds[keep], K, 3, True, "beside an asymmetric instance", u=u[keep])
    with pytest.raises(ValueError, match=r"instances \[2\] are not bitwise symmetric"):
        ops.ils(t, c, Db, K, u=dev(u))


def test_outputs_are_fully_written_and_unrun_trace_entries_stay():
    from gnngls_amd import _lib
    Ds, D, t, c, tours, costs = load(33)
    B, n, K = len(Ds), 33, 12
    u = np.random.default_rng(7).random((B, K, 3))
    cap = host.ils(tours[0], costs[0], Ds[0], 3, u=u[0][:3])[2]            # the moves of three kicks: later kicks never run
    tour_out = torch.full((B, n + 1), -7, dtype=torch.int32, device=D.device)
    cost_out = torch.full((B,), SENTINEL, dtype=torch.float64, device=D.device)
    moves, acc, st = (torch.full((B,), -7, dtype=torch.int32, device=D.device) for _ in range(3))
    trace = torch.full((B, K), SENTINEL, dtype=torch.float64, device=D.device)
    ud = dev(u)
    _lib.check(_lib.load().gnngls_ils_run(_lib.ptr(t), _lib.ptr(c), _lib.ptr(D), B, n, K, 0, 3, 1, cap, 0, _lib.ptr(ud), _lib.ptr(tour_out),
                                          _lib.ptr(cost_out), _lib.ptr(moves), _lib.ptr(acc), _lib.ptr(st), _lib.ptr(trace),
                                          _lib.current_stream()), "ils_run")
    torch.cuda.synchronize()
    assert (tour_out >= 0).all() and (cost_out > 0).all() and (moves >= 0).all() and (acc >= 0).all() and (st >= 0).all()
    some_unrun = False
    for b in range(B):
        w = host.ils(tours[b], costs[b], Ds[b], K, max_moves=cap, u=u[b])
        assert tour_out[b].tolist() == w[0] and bits(cost_out.cpu().numpy()[b]) == bits(w[1])
        assert (int(moves[b]), int(acc[b]), int(st[b])) == w[2:5]
        row = trace[b].cpu().numpy()
        assert np.array_equal(bits(row[:len(w[5])]), bits(w[5])) and (row[len(w[5]):] == SENTINEL).all()
        some_unrun |= len(w[5]) < K
    assert some_unrun


def test_largest_instance():
    from gnngls_amd import ops
    Ds, D, t, c, tours, costs = load(1024, 1)
    r = ops.ils(t, c, D, 1, seed=3, want_trace=True)
    d = ops.or_opt_descent(t, c, D)
    row = r.tour[0].tolist()
    assert row[0] == row[-1] == 0 and sorted(row[:-1]) == list(range(1024))
    assert float(r.cost[0]) <= float(d.cost[0]) and int(r.status[0]) == 0 and int(r.moves[0]) >= int(d.moves[0])
    assert abs(float(r.cost[0]) - sum(Ds[0][x, y] for x, y in zip(row[:-1], row[1:]))) <= 1e-9 * float(r.cost[0])
    assert float(r.trace_cost[0, 0]) >= float(r.cost[0])


def test_a_large_instance_equals_the_host_definition():
    """n = 513 against host.ils: sixteen wavefronts, nine landing blocks.  Two kicks from the descent's local optimum (what
    ops.or_opt_descent leaves: here an input, a closed permutation) -- the first with p1 = 1 and p3 = n - 1, the outermost cuts --
    under a cap of 20 moves: by the host definition the two repairs take 24 moves (0.8 s on the host), so the cap ends the second."""
    from gnngls_amd import ops
    n = 513
    Ds, D, t, c, tours, costs = load(n, 1)
    d = ops.or_opt_descent(t, c, D)
    start = d.tour[0].tolist()
    assert start[0] == start[-1] == 0 and sorted(start[:-1]) == list(range(n)) and int(d.status[0]) == 0
    u = np.array([[[0.0, 0.5, U_MAX], [0.37, 0.52, 0.81]]])
    assert host.double_bridge_cuts(u[0, 0], n) == (1, 257, n - 1)
    r = ops.ils(d.tour, d.cost, D, 2, 3, True, max_moves=20, u=dev(u), want_trace=True)
    want = assert_ils(r, [start], d.cost.cpu().numpy(), Ds, 2, 3, True, "n=513 max_moves=20", u=u, max_moves=20)
    assert want[0][2:5] == (20, 0, host.ILS_STATUS_MOVE_CAP) and len(want[0][5]) == 2     # both kicks ran, the first was repaired


def test_mirror_and_torch_operator_return_what_ops_returns():
    from gnngls_amd import algorithms, ops
    import gnngls_amd.torch_ops  # noqa: F401
    Ds, D, t, c, tours, costs = load(33)
    K, seed = 8, 99
    r = ops.ils(t, c, D, K, seed=seed, want_trace=True)
    tour, cost, moves, acc, st, trace = torch.ops.gnngls.ils(t, c, D, K, 0, 3, True, 100 * 33 * (K + 1), seed, None)
    for got, f in ((tour, "tour"), (cost, "cost"), (moves, "moves"), (acc, "accepted"), (st, "status"), (trace, "trace_cost")):
        assert same_bits(got, getattr(r, f)), f
    # the mirror runs instance 0 of a batch of one: the draws of b = 0
    one = ops.ils(t[:1].contiguous(), c[:1].contiguous(), D[:1].contiguous(), K, seed=seed, want_trace=True)
    mt, mc, per_kick = algorithms.iterated_local_search(tours[0], costs[0], Ds[0], K, seed=seed)
    assert mt == one.tour[0].tolist() and bits(mc) == bits(one.cost.cpu().numpy()[0])
    assert np.array_equal(bits(per_kick), bits(one.trace_cost.cpu().numpy()[0]))
    # seed=None: one draw from NumPy's global stream
    np.random.seed(11)
    a = algorithms.iterated_local_search(tours[0], costs[0], Ds[0], K)
    after = np.random.random()
    np.random.seed(11)
    s = algorithms._draw_seed(None)
    assert after == np.random.random()
    b = algorithms.iterated_local_search(tours[0], costs[0], Ds[0], K, seed=s)
    assert a[0] == b[0] and bits(a[1]) == bits(b[1])
