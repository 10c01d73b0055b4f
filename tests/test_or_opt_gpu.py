"""GPU checks of Or-opt (gnngls_or_opt_best_move, gnngls_or_opt_descent; oropt_kernels.hip) against the NumPy restatement of its
definition in gnngls_amd.host (itself pinned to brute force and to the reference's goldens in tests/test_or_opt_cpu.py): equality
always means equal bit patterns of every fp64 value and equal tours.  Instances are euclid(default_rng(1000 + n), n) from the
nearest-neighbour start, as in the bound's and alpha's tests.  Then the reduction to the reference on the device (max_seg=1 without
reversal is the persistent search kernel's local_search), and the plumbing: solve_batch(polish="or_opt"), the per-call mirrors, the
command line and the torch operator."""
import json
import os
import pickle
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(ROOT, "tests"))

from gnngls_amd import host  # noqa: E402
from test_alpha_cpu import tie_heavy  # noqa: E402
from test_one_tree_cpu import euclid  # noqa: E402
from test_or_opt_cpu import SETTINGS, bits  # noqa: E402

# nothing to move (3: one cycle), a handful of candidates (4, 5), the wavefront's edges, and one to sixteen wavefronts per instance
# (one per 16 nodes: the arg-min's one-barrier form up to eight of them at n = 128, its two-step form from n = 129)
SIZES = (3, 4, 5, 8, 20, 63, 64, 65, 100, 128, 129, 200, 257)
BIG = (513, 1024)


def dev(x, dtype=torch.float64):
    from gnngls_amd import ops
    return ops.as_dev(np.asarray(x), dtype)


_cache = {}


def load(n, count=3):
    """-> (Ds [count,n,n], D on the device, nearest-neighbour tours on the device, their costs, the tours as lists, the costs
    as floats); built once per size."""
    from gnngls_amd import ops
    if (n, count) not in _cache:
        rng = np.random.default_rng(1000 + n)
        Ds = np.stack([euclid(rng, n) for _ in range(count)])
        D = dev(Ds)
        t = ops.nearest_neighbor(D)
        c = ops.tour_cost(t, D)
        _cache[n, count] = (Ds, D, t, c, t.cpu().numpy().tolist(), c.cpu().numpy())
    return _cache[n, count]


def assert_scan(got, tours, Ds, max_seg, reverse, what):
    delta, move, new = (x.cpu().numpy() for x in got)
    for b, (tour, D) in enumerate(zip(tours, Ds)):
        wd, wm = host.or_opt_a2a(tour, D, max_seg, reverse)
        assert move[b].tolist() == (list(wm) if wm else [-1] * 4), (what, b, move[b].tolist(), wm)
        assert bits(delta[b]) == bits(float(wd)), (what, b, delta[b], wd)
        assert new[b].tolist() == (host.or_opt(tour, *wm) if wm else tour), (what, b)


def assert_descent(r, tours, costs, Ds, max_seg, reverse, what, max_moves=None):
    tour, cost, moves, st = r.tour.cpu().numpy(), r.cost.cpu().numpy(), r.moves.cpu().numpy(), r.status.cpu().numpy()
    trace = None if r.trace_cost is None else r.trace_cost.cpu().numpy()
    for b, D in enumerate(Ds):
        wt, wc, wm, wtr = host.or_opt_descent(tours[b], costs[b], D, max_seg, reverse, max_moves)
        assert int(moves[b]) == wm, (what, b, int(moves[b]), wm)
        assert tour[b].tolist() == wt, (what, b)
        assert bits(cost[b]) == bits(wc), (what, b, cost[b], wc)
        # the cap is checked after every move: MOVE_CAP exactly where the host definition applied max_moves moves
        assert int(st[b]) == (6 if wm == max_moves else 0), (what, b, int(st[b]))
        if trace is not None:
            assert wm <= trace.shape[1] and np.array_equal(bits(trace[b, :wm]), bits(wtr)), (what, b)
            assert not trace[b, wm:].any(), (what, b)
    return moves


@pytest.mark.parametrize("n", SIZES)
def test_one_scan_equals_the_host_definition(n):
    from gnngls_amd import ops
    Ds, D, t, c, tours, costs = load(n)
    found = 0
    for max_seg, reverse in SETTINGS:
        got = ops.or_opt_best_move(t, D, max_seg, reverse)
        assert_scan(got, tours, Ds, max_seg, reverse, f"n={n} max_seg={max_seg} reverse={reverse}")
        found += int((got[1][:, 0] >= 0).sum())
    assert (found == 0) == (n == 3), (n, found)          # three nodes have one cycle; by the host definition the larger tours move
    # and from a tour that is no greedy walk: the later scans of a descent see these
    rng = np.random.default_rng(7000 + n)
    perm = [[0] + (rng.permutation(n - 1) + 1).tolist() + [0] for _ in Ds]
    assert_scan(ops.or_opt_best_move(dev(perm, torch.int32), D, 3, True), perm, Ds, 3, True, f"n={n} random tours")


@pytest.mark.parametrize("n", BIG)
def test_one_scan_at_the_large_sizes(n):
    from gnngls_amd import ops
    Ds, D, t, c, tours, costs = load(n, 1)
    assert_scan(ops.or_opt_best_move(t, D, 3, True), tours, Ds, 3, True, f"n={n}")


@pytest.mark.parametrize("n", SIZES)
def test_descent_equals_the_host_definition(n):
    from gnngls_amd import ops
    Ds, D, t, c, tours, costs = load(n)
    for max_seg, reverse in SETTINGS:
        r = ops.or_opt_descent(t, c, D, max_seg, reverse, trace_cap=max(2 * n, 8))
        moves = assert_descent(r, tours, costs, Ds, max_seg, reverse, f"n={n} max_seg={max_seg} reverse={reverse}")
        assert (moves.sum() == 0) == (n == 3)
    # without a trace buffer, and with one shorter than the run: the same result, the first entries of the trace
    r0 = ops.or_opt_descent(t, c, D)
    assert r0.trace_cost is None and torch.equal(r0.tour, r.tour) and torch.equal(r0.cost, r.cost) and torch.equal(r0.moves, r.moves)
    if n >= 20:
        r1 = ops.or_opt_descent(t, c, D, trace_cap=2)
        assert torch.equal(r1.tour, r.tour) and torch.equal(r1.trace_cost, r.trace_cost[:, :2])


@pytest.mark.parametrize("n", BIG)
def test_descent_at_the_large_sizes_under_a_move_cap(n):
    from gnngls_amd import ops
    Ds, D, t, c, tours, costs = load(n, 1)
    r = ops.or_opt_descent(t, c, D, 3, True, max_moves=8, trace_cap=8)
    assert_descent(r, tours, costs, Ds, 3, True, f"n={n} max_moves=8", max_moves=8)
    assert r.moves.tolist() == [8] and r.status.tolist() == [ops.STATUS_MOVE_CAP]


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5])
def test_move_cap_stops_after_k_moves(k):
    from gnngls_amd import ops
    Ds, D, t, c, tours, costs = load(20)
    r = ops.or_opt_descent(t, c, D, 3, True, max_moves=k, trace_cap=8)
    assert_descent(r, tours, costs, Ds, 3, True, f"n=20 max_moves={k}", max_moves=k)
    # by the host definition the three descents take 2, 6 and 4 moves: the cap ends those that would take k or more
    assert r.moves.tolist() == [min(k, m) for m in (2, 6, 4)]
    assert r.status.tolist() == [ops.STATUS_MOVE_CAP if k <= m else 0 for m in (2, 6, 4)]


def test_move_cap_status_even_at_a_local_optimum():
    """The cap is checked after every move: a run whose last allowed move reaches the local optimum still reports MOVE_CAP, one
    more allowed move reports OK with the same tour."""
    from gnngls_amd import ops
    Ds, D, t, c, tours, costs = load(20)
    full = ops.or_opt_descent(t, c, D)
    assert full.status.tolist() == [0, 0, 0]
    for b in range(3):
        m = int(full.moves[b])
        at = ops.or_opt_descent(t[b:b + 1], c[b:b + 1], D[b:b + 1], max_moves=m)
        over = ops.or_opt_descent(t[b:b + 1], c[b:b + 1], D[b:b + 1], max_moves=m + 1)
        assert at.status.tolist() == [ops.STATUS_MOVE_CAP] and over.status.tolist() == [ops.STATUS_OK]
        assert torch.equal(at.tour, full.tour[b:b + 1]) and torch.equal(over.tour, full.tour[b:b + 1])
        assert torch.equal(at.cost, full.cost[b:b + 1])


@pytest.mark.parametrize("n", [8, 20, 50, 100])
def test_single_node_descent_is_the_reference_local_search(n):
    from gnngls_amd import ops
    z = np.load(os.path.join(GOLDEN, f"ls_n{n}.npz"))
    Ds, D, t, c, tours, costs = load(n)
    # the goldens' instance joins the batch
    Dg = torch.cat([D, dev(z["D"][None])])
    tg = torch.cat([t, dev(z["fi0_init_tour"][None], torch.int32)])
    cg = torch.cat([c, dev(z["fi0_init_cost"][None])])
    r = ops.or_opt_descent(tg, cg, Dg, max_seg=1, reverse=False, trace_cap=len(z["fi0_trace"]) + 1)
    g = ops.gls_run(Dg, None, tg, cg, max_outer_iters=0)
    assert torch.equal(r.tour, g.best_tour) and torch.equal(r.cost.view(torch.int64), g.best_cost.view(torch.int64))
    assert r.tour[3].tolist() == z["fi0_tour"].tolist() and bits(float(r.cost[3])) == bits(z["fi0_cost"])
    assert int(r.moves[3]) == len(z["fi0_trace"])
    assert np.array_equal(bits(r.trace_cost[3, :-1].cpu().numpy()), bits(z["fi0_trace"])) and float(r.trace_cost[3, -1]) == 0.0


@pytest.mark.parametrize("n", [20, 100])
def test_tie_heavy_integer_matrices(n):
    from gnngls_amd import ops
    rng = np.random.default_rng(2000 + n)
    Ds = np.stack([tie_heavy(rng, n) for _ in range(3)])
    D = dev(Ds)
    t = ops.nearest_neighbor(D)
    c = ops.tour_cost(t, D)
    tours, costs = t.cpu().numpy().tolist(), c.cpu().numpy()
    for max_seg, reverse in ((1, False), (2, True), (3, True)):
        what = f"ties n={n} max_seg={max_seg} reverse={reverse}"
        assert_scan(ops.or_opt_best_move(t, D, max_seg, reverse), tours, Ds, max_seg, reverse, what)
        assert_descent(ops.or_opt_descent(t, c, D, max_seg, reverse, trace_cap=4 * n), tours, costs, Ds, max_seg, reverse, what)


def test_batch_independence():
    from gnngls_amd import ops
    Ds, D, t, c, tours, costs = load(50, 5)
    batch = ops.or_opt_descent(t, c, D, trace_cap=100)
    alone = ops.or_opt_descent(t[2:3], c[2:3], D[2:3], trace_cap=100)
    for name in ("tour", "cost", "moves", "status", "trace_cost"):
        assert torch.equal(getattr(batch, name)[2:3], getattr(alone, name)), name
    assert_descent(alone, tours[2:3], costs[2:3], Ds[2:3], 3, True, "n=50 alone")
    sb, sa = ops.or_opt_best_move(t, D), ops.or_opt_best_move(t[2:3], D[2:3])
    assert all(torch.equal(x[2:3], y) for x, y in zip(sb, sa))


def test_asymmetric_matrix_is_flagged():
    from gnngls_amd import _lib, ops
    Ds, _, t, c, tours, costs = load(20, 4)
    Ds = Ds.copy()
    Ds[2, 7, 11] = np.nextafter(Ds[2, 7, 11], np.inf)  # one ulp in one triangle
    D = dev(Ds)
    with pytest.raises(ValueError, match=r"instances \[2\].*symmetric"):
        ops.or_opt_descent(t, c, D)
    with pytest.raises(ValueError, match=r"instances \[2\].*symmetric"):
        ops.or_opt_best_move(t, D)
    tour_out = torch.full((4, 21), -7, dtype=torch.int32, device="cuda")
    cost_out = torch.full((4,), -7.0, dtype=torch.float64, device="cuda")
    moves = torch.full((4,), -7, dtype=torch.int32, device="cuda")
    status = torch.full((4,), -7, dtype=torch.int32, device="cuda")
    trace = torch.zeros((4, 64), dtype=torch.float64, device="cuda")
    assert _lib.load().gnngls_or_opt_descent(_lib.ptr(t), _lib.ptr(c), _lib.ptr(D), 4, 20, 3, 1, 2000, _lib.ptr(tour_out), _lib.ptr(cost_out),
                                             _lib.ptr(moves), _lib.ptr(status), _lib.ptr(trace), 64, _lib.current_stream()) == 0
    torch.cuda.synchronize()
    assert status.tolist() == [0, 0, ops.STATUS_ASYMMETRIC, 0]
    assert torch.equal(tour_out[2], t[2]) and torch.equal(cost_out[2].view(torch.int64), c[2].view(torch.int64)) and int(moves[2]) == 0
    assert not bool(trace[2].any())
    ok = [0, 1, 3]
    r = ops.OrOptResult(tour_out[ok], cost_out[ok], moves[ok], status[ok], trace[ok])
    assert_descent(r, [tours[b] for b in ok], costs[ok], Ds[ok], 3, True, "the symmetric instances of the batch")


def uniform_instances(n=100, count=8):
    """The recipe the polish was prototyped on: uniform points, rng keyed by 1000 + n + s."""
    out = []
    for s in range(count):
        xy = np.random.default_rng(1000 + n + s).random((n, 2))
        out.append(np.sqrt(((xy[:, None] - xy[None]) ** 2).sum(-1)))
    return np.stack(out)


def test_polish_plumbing():
    from gnngls_amd import ops, pipeline
    Ds = uniform_instances()
    D = dev(Ds)
    plain = pipeline.solve_batch(D, guides=("weight",), max_outer_iters=0)
    assert plain.polish_gain is None and "polish_s" not in plain.timing
    res = pipeline.solve_batch(D, guides=("weight",), max_outer_iters=0, polish="or_opt")
    want = ops.or_opt_descent(plain.best_tour, plain.best_cost, D)
    assert torch.equal(res.best_tour, want.tour) and torch.equal(res.best_cost.view(torch.int64), want.cost.view(torch.int64))
    assert torch.equal(res.polish_gain, plain.best_cost - want.cost) and bool((res.polish_gain >= 0).all())
    assert res.timing["polish_s"] > 0
    # from the host definition: the 2-opt + relocate optimum of at least one of these instances is no Or-opt optimum
    tours, costs = plain.best_tour.cpu().numpy().tolist(), plain.best_cost.cpu().numpy()
    moved = [host.or_opt_descent(tours[b], costs[b], Ds[b])[2] > 0 for b in range(len(Ds))]
    assert sum(moved) >= 1, moved
    assert ((res.polish_gain > 0).cpu().numpy() == np.array(moved)).all()
    assert_descent(want, tours, costs, Ds, 3, True, "polish of the local optima")
    # a shorter chain is another descent
    seg1 = pipeline.solve_batch(D, guides=("weight",), max_outer_iters=0, polish="or_opt", polish_seg=1)
    assert torch.equal(seg1.best_tour, ops.or_opt_descent(plain.best_tour, plain.best_cost, D, 1).tour)
    # multi-start: the winner is polished; with a bound: it is computed on the polished cost
    many_plain = pipeline.solve_batch(D, guides=("weight",), max_outer_iters=0, starts=3)
    many = pipeline.solve_batch(D, guides=("weight",), max_outer_iters=0, starts=3, polish="or_opt")
    assert bool((many.best_cost <= many_plain.best_cost).all()) and torch.equal(many.best_start, many_plain.best_start)
    assert torch.equal(many.polish_gain, many_plain.best_cost - many.best_cost)
    lb = pipeline.solve_batch(D, guides=("weight",), max_outer_iters=0, polish="or_opt", lower_bound=True, bound_iters=200)
    assert torch.equal(lb.best_cost, res.best_cost) and bool((lb.lower_bound <= lb.best_cost).all())
    assert torch.equal(lb.lower_bound, ops.one_tree_bound(D, res.best_cost, max_iters=200, want_pi=False).bound)
    with pytest.raises(ValueError, match="polish_seg"):
        pipeline.solve_batch(D, guides=("weight",), max_outer_iters=0, polish="or_opt", polish_seg=4)


def test_single_graph_mirrors():
    import gnngls_amd
    from gnngls_amd import algorithms, datasets, operators, ops
    from gnngls_amd.algorithms import _attr_matrix
    from test_n3_ingestion_cpu import names
    G = datasets.read_gpickle(os.path.join(ROOT, "tests", "golden", "n3_tsp12", names()[0]))
    Dm = _attr_matrix(G, "weight")
    D = dev(Dm[None])
    init = algorithms.nearest_neighbor(G, 0)
    cost = gnngls_amd.tour_cost(G, init)
    t = dev([init], torch.int32)
    for max_seg, reverse in ((3, True), (2, False), (1, False)):
        delta, new = operators.or_opt_a2a(init, Dm, max_seg, reverse)
        d, mv, nt = ops.or_opt_best_move(t, D, max_seg, reverse)
        assert new == nt[0].tolist() and bits(float(delta)) == bits(float(d[0]))
        if delta < 0:
            assert bits(operators.or_opt_cost(init, Dm, *mv[0].tolist())) == bits(float(delta))
            assert operators.or_opt(init, *mv[0].tolist()) == new
        tour, c, moves = algorithms.or_opt_descent(init, cost, Dm, max_seg, reverse)
        r = ops.or_opt_descent(t, dev([cost]), D, max_seg, reverse)
        assert tour == r.tour[0].tolist() and bits(c) == bits(float(r.cost[0])) and moves == int(r.moves[0])
        assert gnngls_amd.is_valid_tour(G, tour) and abs(c - gnngls_amd.tour_cost(G, tour)) <= 1e-9 * c
    ls_tour, ls_cost, _ = algorithms.local_search(init, cost, Dm)
    assert (tour, bits(c)) == (ls_tour, bits(ls_cost))               # the last setting is the reference's descent


def test_torch_op():
    import gnngls_amd.torch_ops  # noqa: F401
    from gnngls_amd import ops
    Ds, D, t, c, tours, costs = load(20)
    for args in ((3, True, 2000, 16), (2, False, 3, 0)):
        tour, cost, moves, status, trace = torch.ops.gnngls.or_opt_descent(t, c, D, *args)
        r = ops.or_opt_descent(t, c, D, *args)
        assert torch.equal(tour, r.tour) and torch.equal(cost, r.cost) and torch.equal(moves, r.moves) and torch.equal(status, r.status)
        assert trace.shape == (3, args[3]) and (r.trace_cost is None or torch.equal(trace, r.trace_cost))


def test_cli_polish(tmp_path):
    fix = os.path.join(ROOT, "tests", "golden", "n3_tsp12")
    data = tmp_path / "tsp12"
    shutil.copytree(fix, data)
    mdir = tmp_path / "models" / "tsp12"
    mdir.mkdir(parents=True)
    json.dump({"embed_dim": 128, "n_layers": 3, "n_heads": 8}, open(mdir / "params.json", "w"))
    run_dir = tmp_path / "runs"
    subprocess.check_call([sys.executable, os.path.join(ROOT, "scripts", "test.py"), str(data / "test.txt"),
                           str(mdir / "checkpoint_best_val.pt"), str(run_dir), "weight", "--time_limit", "0.2", "--use_gpu",
                           "--polish", "or_opt"], cwd=ROOT)
    df = pickle.load(open(next(run_dir.glob("*.pkl")), "rb"))
    assert list(df.columns) == ["instance", "time", "opt_cost", "cost", "best_cost", "gap", "dt"]
    assert (df.groupby("instance")["gap"].last() >= -1e-7).all()
