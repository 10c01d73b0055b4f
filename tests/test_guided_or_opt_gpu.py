"""GPU checks of guided local search over 2-opt and Or-opt (gnngls_or_opt_o2a, gnngls_guided_or_opt_run; or_opt_o2a_kernel and
guided_or_opt_kernel in oropt_kernels.hip) against the NumPy restatement of the definition in gnngls_amd.host (itself pinned in
tests/test_guided_or_opt_cpu.py, which also asserts that these seeds exercise every kind of move) and, with chains of one node,
against gls_run: equality always means equal bit patterns of every fp64 value, equal tours and equal penalties.  Instances are
euclid(default_rng(1000 + n), n) from the nearest-neighbour start, as in the Or-opt tests; beyond n = 129 (241 to 1024: sixteen
wavefronts, several landing blocks per chain, the selection key's fields full) one instance per size, the run from the descent's
local optimum.  Matrices that are no well-scaled distances are in tests/test_search_fuzz_gpu.py."""
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
from test_guided_or_opt_cpu import GPU_SIZES as SIZES, K, PM, gpu_guides, gpu_instances, k_of  # noqa: E402
from test_or_opt_cpu import bits  # noqa: E402

# the single 2-opt pair (4), a handful (5, 6, 9), two and three wavefronts (17, 33), the lane loop's edge (64, 65), 100, and the
# two-step arg-min (129: nine wavefronts)
SETTINGS = [(1, False), (3, True)]
SENTINEL = -12345.0
CAP = 512                                                       # trace entries: more than any run here applies
FIELDS = ("tour", "cost", "best_tour", "best_cost", "moves", "steps", "status", "penalty", "trace_cost", "trace_len")


def dev(x, dtype=torch.float64):
    from gnngls_amd import ops
    return ops.as_dev(np.asarray(x), dtype)


def same_bits(a, b):
    return torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a, b.view(torch.int64) if b.dtype == torch.float64 else b)


_cache = {}


def load(n):
    """-> (Ds, guides [2,B,n,n], D and the guides on the device, nearest-neighbour tours on the device, their costs, the tours as
    lists, the costs as floats); built once per size."""
    from gnngls_amd import ops
    if n not in _cache:
        Ds = gpu_instances(n)
        gs = gpu_guides(Ds, n)
        D = dev(Ds)
        t = ops.nearest_neighbor(D)
        c = ops.tour_cost(t, D)
        _cache[n] = (Ds, gs, D, dev(gs), t, c, t.cpu().numpy().tolist(), c.cpu().numpy())
    return _cache[n]


_want = {}


def host_run(n, max_seg, reverse):
    """host.guided_or_opt of every instance of size n for K iterations, computed once: [(result, penalties)]."""
    if (n, max_seg, reverse) not in _want:
        Ds, gs, D, g, t, c, tours, costs = load(n)
        rows = []
        for b in range(len(Ds)):
            pen = np.zeros((n, n), dtype=np.int32)
            rows.append((host.guided_or_opt(tours[b], costs[b], Ds[b], gs[:, b], K, k_of(costs[b], n), pen, PM, max_seg, reverse), pen))
        _want[n, max_seg, reverse] = rows
    return _want[n, max_seg, reverse]


def assert_run(r, want, what, trace_fill=0.0):
    """Every output of a launch against (host result, host penalties) per instance; the trace's tail must be as given."""
    tour, cost, btour, bcost, moves, steps, st, pen, tlen = (x.cpu().numpy() for x in (r.tour, r.cost, r.best_tour, r.best_cost, r.moves,
                                                                                       r.steps, r.status, r.penalty, r.trace_len))
    trace = r.trace_cost.cpu().numpy()
    for b, (w, wpen) in enumerate(want):
        assert tour[b].tolist() == w[0] and btour[b].tolist() == w[2], (what, b)
        assert bits(cost[b]) == bits(w[1]) and bits(bcost[b]) == bits(w[3]), (what, b, cost[b], w[1], bcost[b], w[3])
        assert (int(moves[b]), int(steps[b]), int(st[b])) == w[4:7], (what, b, moves[b], steps[b], st[b], w[4:7])
        ran = min(len(w[7]), trace.shape[1])
        assert int(tlen[b]) == ran and np.array_equal(bits(trace[b, :ran]), bits(w[7][:ran])), (what, b)
        assert (trace[b, ran:] == trace_fill).all(), (what, b)
        assert np.array_equal(pen[b], wpen), (what, b)


def positions(n, B):
    return [1, n - 1, (n + 1) // 2][:B] if B >= 3 else [1, n - 1]


@pytest.mark.parametrize("n", SIZES)
def test_one_to_all_scan_equals_the_host_scan(n):
    from gnngls_amd import ops
    Ds, gs, D, g, t, c, tours, costs = load(n)
    B = len(Ds)
    found = 0
    # the nearest-neighbour start, and the tour a descent of two moves leaves (other neighbours around every position)
    starts = [(t, tours)]
    d = ops.or_opt_descent(t, c, D, max_moves=2)
    starts.append((d.tour, d.tour.cpu().numpy().tolist()))
    for td, tl in starts:
        for shift in range(3):
            pos = [1 + (p - 1 + shift * ((n - 1) // 3 + 1)) % (n - 1) for p in positions(n, B)]
            for max_seg, reverse in SETTINGS:
                delta, move, new = ops.or_opt_o2a(td, D, dev(pos, torch.int32), max_seg, reverse)
                delta, move, new = delta.cpu().numpy(), move.cpu().numpy(), new.cpu().numpy()
                for b in range(B):
                    wd, wm = host.or_opt_o2a(tl[b], Ds[b], pos[b], max_seg, reverse)
                    assert bits(delta[b]) == bits(float(wd)), (n, b, pos[b], max_seg, delta[b], wd)
                    assert move[b].tolist() == (list(wm) if wm else [-1] * 4), (n, b, pos[b], move[b], wm)
                    assert new[b].tolist() == (host.or_opt(tl[b], *wm) if wm else tl[b])
                    found += wm is not None
    assert found > 0 or n <= 5
    with pytest.raises(ValueError, match="positions must be in"):
        ops.or_opt_o2a(t, D, dev([0] * B, torch.int32))


@pytest.mark.parametrize("n", SIZES)
def test_run_equals_the_host_definition(n):
    from gnngls_amd import ops
    Ds, gs, D, g, t, c, tours, costs = load(n)
    # the default k is the reference's, as Python evaluates it
    for max_seg, reverse in SETTINGS:
        r = ops.guided_or_opt(t, c, D, g, K, perturbation_moves=PM, max_seg=max_seg, reverse=reverse, trace_cap=CAP)
        assert np.array_equal(bits(r.k.cpu().numpy()), bits(np.array([k_of(x, n) for x in costs])))
        assert_run(r, host_run(n, max_seg, reverse), f"n={n} max_seg={max_seg} reverse={reverse}")
    # without a trace buffer: the same result
    r0 = ops.guided_or_opt(t, c, D, g, K, perturbation_moves=PM, max_seg=max_seg, reverse=reverse)
    assert r0.trace_cost is None and not r0.trace_len.any()
    assert all(same_bits(getattr(r0, f), getattr(r, f)) for f in FIELDS[:8])


@pytest.mark.parametrize("n", [33, 100, 129])
def test_chains_of_one_node_are_gls_run(n):
    from gnngls_amd import ops
    Ds, gs, D, g, t, c, tours, costs = load(n)
    r = ops.guided_or_opt(t, c, D, g, K, perturbation_moves=PM, max_seg=1, reverse=False, trace_cap=CAP)
    o = ops.gls_run(D, g, t, c, perturbation_moves=PM, max_outer_iters=K, want_penalty=True, trace_cap=CAP)
    assert torch.equal(r.best_tour, o.best_tour) and same_bits(r.best_cost, o.best_cost)
    assert torch.equal(r.penalty, o.penalty) and not r.status.any() and not o.status.any()
    assert torch.equal(r.moves, o.trace_len) and same_bits(r.trace_cost, o.trace_cost)


def test_beyond_the_lds_resident_stores_it_is_gls_run_on_global_memory():
    """n = 300: no Python definition is run at this size."""
    from gnngls_amd import ops
    n = 300
    Ds = gpu_instances(n)[:1]
    D, g = dev(Ds), dev(gpu_guides(Ds, n))
    t = ops.nearest_neighbor(D)
    c = ops.tour_cost(t, D)
    assert ops.gls_resident_capacity(n) == 0
    r = ops.guided_or_opt(t, c, D, g, 1, perturbation_moves=5, max_seg=1, reverse=False, trace_cap=CAP)
    o = ops.gls_run(D, g, t, c, perturbation_moves=5, max_outer_iters=1, want_penalty=True, trace_cap=CAP)
    assert torch.equal(r.best_tour, o.best_tour) and same_bits(r.best_cost, o.best_cost) and torch.equal(r.penalty, o.penalty)
    assert torch.equal(r.moves, o.trace_len) and same_bits(r.trace_cost, o.trace_cost) and int(r.steps[0]) >= 2 and not r.status.any()


def load_large(n):
    """One instance of the sizes beyond SIZES: -> (Ds [1,n,n], guides [2,1,n,n], D and the guides on the device, the
    nearest-neighbour tour on the device, its cost); built once per size."""
    from gnngls_amd import ops
    if ("large", n) not in _cache:
        Ds = gpu_instances(n)[:1]
        gs = gpu_guides(Ds, n)
        D = dev(Ds)
        t = ops.nearest_neighbor(D)
        _cache["large", n] = (Ds, gs, D, dev(gs), t, ops.tour_cost(t, D))
    return _cache["large", n]


@pytest.mark.parametrize("n", [241, 257, 513, 1000, 1024])
def test_one_to_all_scan_at_the_large_sizes(n):
    """From n = 241 every instance runs sixteen wavefronts and the landing blocks of a chain (ceil(n / 64), sixteen at n = 1024) go
    round them; at n = 1024 the ten-bit fields of the selection key are full.  Positions: the ends, the middle, and every multiple
    of 64 with its two neighbours (the blocks' edges)."""
    from gnngls_amd import ops
    Ds, gs, D, g, t, c = load_large(n)
    tour = t[0].tolist()
    pos = {1, 2, 3, n - 3, n - 2, n - 1, (n + 1) // 2} | {m + d for m in range(64, n, 64) for d in (-1, 0, 1)}
    pos = sorted(p for p in pos if 1 <= p <= n - 1)
    assert n - 1 in pos and (n < 1024 or 1023 in pos)
    found = chains = 0
    for max_seg, reverse in SETTINGS:
        got = [ops.or_opt_o2a(t, D, dev([p], torch.int32), max_seg, reverse) for p in pos]
        for p, (delta, move, new) in zip(pos, got):
            wd, wm = host.or_opt_o2a(tour, Ds[0], p, max_seg, reverse)
            assert move[0].tolist() == (list(wm) if wm else [-1] * 4), (n, p, max_seg, move[0].tolist(), wm)
            assert bits(delta.cpu().numpy()[0]) == bits(float(wd)), (n, p, max_seg, float(delta[0]), wd)
            assert new[0].tolist() == (host.or_opt(tour, *wm) if wm else tour), (n, p, max_seg)
            found += wm is not None
            chains += wm is not None and wm[1] >= 2
    assert found > 0 and chains > 0


@pytest.mark.parametrize("n", [241, 300, 513, 1024])
def test_run_at_the_large_sizes(n):
    """The run against the host definition beyond n = 129, K = 2 iterations of 5 moves from a local optimum: a full host descent
    from the nearest-neighbour tour takes hundreds of scans at these sizes, so the start tour is what ops.or_opt_descent leaves
    (checked against the host on its own in tests/test_or_opt_gpu.py; here it is an input: a closed permutation, its cost summed
    left to right).  With chains of one node the run is gls_run's, which accepts every one of these sizes (global-memory store).
    By the host's log the seeds of 513 and 1024 apply 2-opt moves and chains of two or three nodes in their penalty steps."""
    from gnngls_amd import ops
    Ds, gs, D, g, t, c = load_large(n)
    K2, PM2 = 2, 5
    for max_seg, reverse in [(3, True), (1, False)]:
        start = ops.or_opt_descent(t, c, D, max_seg, reverse).tour
        tour = start[0].tolist()
        assert tour[0] == tour[-1] == 0 and sorted(tour[:-1]) == list(range(n))
        cost = 0.0
        for x, y in zip(tour[:-1], tour[1:]):
            cost = cost + Ds[0][x, y]
        c0 = dev([cost])
        r = ops.guided_or_opt(start, c0, D, g, K2, perturbation_moves=PM2, max_seg=max_seg, reverse=reverse, trace_cap=CAP)
        pen, log = np.zeros((n, n), dtype=np.int32), []
        w = host.guided_or_opt(tour, cost, Ds[0], gs[:, 0], K2, k_of(cost, n), pen, PM2, max_seg, reverse, log=log)
        assert w[6] == 0 and len(log) >= K2 * PM2
        assert_run(r, [(w, pen)], f"n={n} max_seg={max_seg} reverse={reverse}")
        assert r.status.tolist() == [0]
        if max_seg == 3:
            two, longer = sum(op == 0 for _, op, _ in log), sum(op == 1 and m[1] >= 2 for _, op, m in log)
            assert two >= 1 and longer >= 1, (n, two, longer)
        else:
            assert ops.gls_describe_config(n, 1)["store"] == "global"
            o = ops.gls_run(D, g, start, c0, perturbation_moves=PM2, max_outer_iters=K2, want_penalty=True, trace_cap=CAP)
            assert torch.equal(r.best_tour, o.best_tour) and same_bits(r.best_cost, o.best_cost) and torch.equal(r.penalty, o.penalty)
            assert torch.equal(r.moves, o.trace_len) and same_bits(r.trace_cost, o.trace_cost) and not o.status.any()


@pytest.mark.parametrize("n", [9, 33, 100])
def test_chained_runs_are_one_run(n):
    from gnngls_amd import ops
    Ds, gs, D, g, t, c, tours, costs = load(n)
    K1, K2 = 1, K - 1
    for max_seg, reverse in SETTINGS:
        whole = ops.guided_or_opt(t, c, D, g, K, perturbation_moves=PM, max_seg=max_seg, reverse=reverse, trace_cap=CAP)
        a = ops.guided_or_opt(t, c, D, g, K1, perturbation_moves=PM, max_seg=max_seg, reverse=reverse, trace_cap=CAP)
        first_pen = a.penalty.clone()
        b = ops.guided_or_opt(a.tour, a.cost, D, g, K2, k=a.k, penalty=a.penalty, perturbation_moves=PM, max_seg=max_seg, reverse=reverse,
                              iter0=K1, trace_cap=CAP)
        assert b.penalty.data_ptr() == a.penalty.data_ptr() and not torch.equal(first_pen, b.penalty)       # updated in place
        assert torch.equal(b.tour, whole.tour) and same_bits(b.cost, whole.cost) and torch.equal(b.penalty, whole.penalty)
        assert torch.equal(a.moves + b.moves, whole.moves) and torch.equal(a.steps + b.steps, whole.steps)
        later = b.best_cost < a.best_cost                        # the better of the two bests under <, ties to the earlier
        assert same_bits(torch.where(later, b.best_cost, a.best_cost), whole.best_cost)
        assert torch.equal(torch.where(later[:, None], b.best_tour, a.best_tour), whole.best_tour)
        for i in range(len(Ds)):
            ma, mb = int(a.moves[i]), int(b.moves[i])
            assert same_bits(torch.cat([a.trace_cost[i, :ma], b.trace_cost[i, :mb]]), whole.trace_cost[i, :ma + mb])


def test_both_caps_end_the_run_where_the_host_does():
    from gnngls_amd import ops
    n = 33
    Ds, gs, D, g, t, c, tours, costs = load(n)
    free = ops.guided_or_opt(t, c, D, g, K, perturbation_moves=PM)
    first = ops.or_opt_descent(t, c, D).moves.tolist()
    fm, fs = free.moves.tolist(), free.steps.tolist()
    assert all(m > d + PM for m, d in zip(fm, first)) and min(fs) > PM

    def want(**kw):
        rows = []
        for b in range(len(Ds)):
            pen = np.zeros((n, n), dtype=np.int32)
            rows.append((host.guided_or_opt(tours[b], costs[b], Ds[b], gs[:, b], K, k_of(costs[b], n), pen, PM, 3, True, **kw), pen))
        return rows
    for cap in (1, min(first), max(first) + 1, max(first) + 5, max(first) + PM + 2, min(fm) - 1, max(fm), max(fm) + 1):
        r = ops.guided_or_opt(t, c, D, g, K, perturbation_moves=PM, max_moves=cap, trace_cap=CAP)
        assert_run(r, want(max_moves=cap), f"max_moves={cap}")
        assert r.moves.tolist() == [min(cap, m) for m in fm]
        assert r.status.tolist() == [ops.STATUS_MOVE_CAP if cap <= m else 0 for m in fm]
    for cap in (1, 2, PM, min(fs) - 1, max(fs), max(fs) + 1):
        r = ops.guided_or_opt(t, c, D, g, K, perturbation_moves=PM, max_steps=cap, trace_cap=CAP)
        assert_run(r, want(max_steps=cap), f"max_steps={cap}")
        assert r.steps.tolist() == [min(cap, s) for s in fs]
        assert r.status.tolist() == [ops.STATUS_STEP_CAP if cap < s else 0 for s in fs]


@pytest.mark.parametrize("n", [12, 33])
def test_tie_heavy_instances(n):
    from gnngls_amd import ops
    rng = np.random.default_rng(4000 + n)
    Ds = np.stack([tie_heavy(rng, n) for _ in range(3)])
    gs = np.stack([Ds, gpu_guides(Ds, n)[1]])
    D, g = dev(Ds), dev(gs)
    t = ops.nearest_neighbor(D)
    c = ops.tour_cost(t, D)
    tours, costs = t.cpu().numpy().tolist(), c.cpu().numpy()
    for max_seg, reverse in SETTINGS:
        r = ops.guided_or_opt(t, c, D, g, K, perturbation_moves=PM, max_seg=max_seg, reverse=reverse, trace_cap=CAP)
        want = []
        for b in range(3):
            pen = np.zeros((n, n), dtype=np.int32)
            want.append((host.guided_or_opt(tours[b], costs[b], Ds[b], gs[:, b], K, k_of(costs[b], n), pen, PM, max_seg, reverse), pen))
        assert_run(r, want, f"ties n={n} max_seg={max_seg}")


def test_an_asymmetric_instance_is_reported_and_the_others_searched():
    from gnngls_amd import ops
    n = 17
    Ds, gs, D, g, t, c, tours, costs = load(n)
    bad = Ds.copy()
    bad[1, 3, 11] = np.nextafter(bad[1, 3, 11], 2.0)
    Db = dev(bad)
    pen = torch.zeros((len(Ds), n, n), dtype=torch.int32, device=D.device)
    r = ops.guided_or_opt_launch(t, c, Db, g, K, penalty=pen, perturbation_moves=PM, trace_cap=CAP)
    assert r.status.tolist() == [0, ops.STATUS_ASYMMETRIC, 0]
    assert torch.equal(r.tour[1], t[1]) and torch.equal(r.best_tour[1], t[1])
    assert bits(r.cost.cpu().numpy()[1]) == bits(costs[1]) and bits(r.best_cost.cpu().numpy()[1]) == bits(costs[1])
    assert int(r.moves[1]) == 0 and int(r.steps[1]) == 0 and int(r.trace_len[1]) == 0 and not pen[1].any() and not r.trace_cost[1].any()
    keep = [0, 2]
    want = host_run(n, 3, True)
    sub = ops.GuidedOrOptResult(*(getattr(r, f)[keep] for f in ("tour", "cost", "best_tour", "best_cost", "moves", "steps", "status", "penalty",
                                                             "k", "trace_cost", "trace_len")))
    assert_run(sub, [want[b] for b in keep], "beside an asymmetric instance")
    with pytest.raises(ValueError, match=r"instances \[1\] are not bitwise symmetric"):
        ops.guided_or_opt(t, c, Db, g, K, perturbation_moves=PM)


@pytest.mark.parametrize("n", [33, 100])
def test_results_do_not_depend_on_the_batch_position(n):
    from gnngls_amd import ops
    Ds, gs, D, g, t, c, tours, costs = load(n)
    B = len(Ds)
    r = ops.guided_or_opt(t, c, D, g, K, perturbation_moves=PM, trace_cap=CAP)
    order = list(range(B))[::-1]
    p = ops.guided_or_opt(t[order].contiguous(), c[order].contiguous(), D[order].contiguous(), g[:, order].contiguous(), K,
                          perturbation_moves=PM, trace_cap=CAP)
    for f in FIELDS:
        assert same_bits(getattr(p, f), getattr(r, f)[order]), f
    one = ops.guided_or_opt(t[1:2].contiguous(), c[1:2].contiguous(), D[1:2].contiguous(), g[:, 1:2].contiguous(), K, perturbation_moves=PM,
                            trace_cap=CAP)
    for f in FIELDS:
        assert same_bits(getattr(one, f), getattr(r, f)[1:2]), f


def test_outputs_are_fully_written_and_unrun_trace_entries_stay():
    from gnngls_amd import _lib
    n = 33
    Ds, gs, D, g, t, c, tours, costs = load(n)
    B = len(Ds)
    tour_out, best_tour = (torch.full((B, n + 1), -7, dtype=torch.int32, device=D.device) for _ in range(2))
    cost_out, best_cost = (torch.full((B,), SENTINEL, dtype=torch.float64, device=D.device) for _ in range(2))
    moves, steps, st, tlen = (torch.full((B,), -7, dtype=torch.int32, device=D.device) for _ in range(4))
    trace = torch.full((B, CAP), SENTINEL, dtype=torch.float64, device=D.device)
    pen = torch.zeros((B, n, n), dtype=torch.int32, device=D.device)
    k = dev([k_of(x, n) for x in costs])
    _lib.check(_lib.load().gnngls_guided_or_opt_run(
        _lib.ptr(t), _lib.ptr(c), _lib.ptr(D), _lib.ptr(g), 2, _lib.ptr(k), _lib.ptr(pen), B, n, K, 0, PM, 3, 1, 10 ** 6, 10 ** 6,
        _lib.ptr(tour_out), _lib.ptr(cost_out), _lib.ptr(best_tour), _lib.ptr(best_cost), _lib.ptr(moves), _lib.ptr(steps), _lib.ptr(st),
        _lib.ptr(trace), CAP, _lib.ptr(tlen), _lib.current_stream()), "guided_or_opt_run")
    torch.cuda.synchronize()
    from gnngls_amd import ops
    r = ops.GuidedOrOptResult(tour_out, cost_out, best_tour, best_cost, moves, steps, st, pen, k, trace, tlen)
    assert_run(r, host_run(n, 3, True), "raw entry", trace_fill=SENTINEL)
    assert (tlen < CAP).all()
    # a trace buffer shorter than the run: the first entries of every row, nothing behind the last row
    short = 7
    flat = torch.full((B * short + 3,), SENTINEL, dtype=torch.float64, device=D.device)
    pen.zero_()
    _lib.check(_lib.load().gnngls_guided_or_opt_run(
        _lib.ptr(t), _lib.ptr(c), _lib.ptr(D), _lib.ptr(g), 2, _lib.ptr(k), _lib.ptr(pen), B, n, K, 0, PM, 3, 1, 10 ** 6, 10 ** 6,
        _lib.ptr(tour_out), _lib.ptr(cost_out), _lib.ptr(best_tour), _lib.ptr(best_cost), _lib.ptr(moves), _lib.ptr(steps), _lib.ptr(st),
        _lib.ptr(flat), short, _lib.ptr(tlen), _lib.current_stream()), "guided_or_opt_run")
    torch.cuda.synchronize()
    assert tlen.tolist() == [short] * B and same_bits(flat[:B * short].view(B, short), trace[:, :short].contiguous())
    assert (flat[B * short:] == SENTINEL).all()

def test_torch_operator_returns_what_ops_returns():
    from gnngls_amd import ops
    import gnngls_amd.torch_ops  # noqa: F401
    Ds, gs, D, g, t, c, tours, costs = load(33)
    r = ops.guided_or_opt(t, c, D, g, K, perturbation_moves=PM, trace_cap=CAP)
    out = torch.ops.gnngls.guided_or_opt(t, c, D, g, K, 0, None, None, PM, 3, True, 0, 0, CAP)
    for got, f in zip(out, FIELDS):
        assert same_bits(got, getattr(r, f)), f
    # functional: given penalties are copied, not updated
    given = r.penalty.clone()
    out2 = torch.ops.gnngls.guided_or_opt(r.tour, r.cost, D, g, 1, K, r.k, given, PM, 3, True, 0, 0, 0)
    assert torch.equal(given, r.penalty) and not torch.equal(out2[7], given) and out2[8].shape == (len(Ds), 0)
