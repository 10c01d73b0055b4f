"""GPU tests of the sampled nearest-neighbour walks (gnngls_sample_nn_tours, reference algorithms.py:21-64) and of the
multi-start search built on them (pipeline.solve_batch(starts=R)).

Equality of tours is exact: given the uniforms, the device walk is the NumPy restatement of tests/test_sampling_cpu.py bit for
bit (same summation order, contraction off).  Against the reference itself the walks agree in law: 20,000 device walks pass
the chi-square bound the reference's own counts pass in the CPU test.

"The same walk launched alone" (generator test): the C entry has no (b, r) offset, so the walk is launched alone with ITS
uniforms -- the restated Philox stream of counter (b, r, .) -- as the explicit `u` of a B = 1, R = 1 launch, and walk (b, r) is
also compared across launches of other shapes that contain it."""
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
FIX = os.path.join(ROOT, "tests", "golden", "n3_tsp12")
sys.path.insert(0, os.path.join(ROOT, "tests"))

from test_insertion_cpu import make_instance  # noqa: E402
from test_sampling_cpu import (BAD_WEIGHTS, LAW_FIXTURE, all_tours, chi_square, chi_square_bound, philox_uniforms,  # noqa: E402
                               restated_walks, tour_probability)

SIZES = (3, 4, 5, 63, 64, 65, 100, 129, 200, 257)


def device_walks(W, R, depot=0, invert=True, seed=0, u=None):
    """The torch op: reports a bad walk in `status` instead of raising -> numpy (tours, status)."""
    import gnngls_amd.torch_ops  # noqa: F401
    Wd = torch.from_numpy(np.ascontiguousarray(W)).cuda()
    ud = None if u is None else torch.from_numpy(np.ascontiguousarray(u)).cuda()
    tours, status = torch.ops.gnngls.sample_nn_tours(Wd, R, depot, invert, seed, ud)
    torch.cuda.synchronize()
    return tours.cpu().numpy(), status.cpu().numpy()


def uniforms(rng, B, R, n):
    u = rng.random((B, R, n - 1))
    u[0, 0, :] = 0.0                                     # the ends of [0, 1)
    u[-1, -1, :] = np.nextafter(1.0, 0.0)
    u[0, -1, ::2] = 0.0
    u[0, -1, 1::2] = np.nextafter(1.0, 0.0)
    return u


def nonmetric(rng, B, n):
    return np.ascontiguousarray(rng.uniform(0.1, 3.0, size=(B, n, n)))        # asymmetric, no triangle inequality


def check_against_restatement(W, depot, invert, u):
    tours, status = device_walks(W, u.shape[1], depot, invert, 0, u)
    ref_tours, ref_status = restated_walks(W, depot, invert, u)
    assert np.array_equal(status, ref_status)
    assert np.array_equal(tours, ref_tours)
    return tours, status


# ---- 1. given u ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_given_u_equals_the_restatement(n):
    rng = np.random.default_rng(1000 + n)
    B, R = 3, 5
    euclid = np.stack([make_instance("euclid", n, rng) for _ in range(B)])
    for W in (euclid, nonmetric(rng, B, n)):
        for invert in (True, False):
            _, status = check_against_restatement(W, int(rng.integers(0, n)), invert, uniforms(rng, B, R, n))
            assert (status == 0).all()
    # many equal weights: the boundaries of the running sums are hit by ties (zero distances: without inversion, and shifted by one with it)
    lattice = make_instance("lattice", n, rng)[None]
    check_against_restatement(lattice, 0, False, uniforms(rng, 1, 3, n))
    _, status = check_against_restatement(lattice + 1.0, n - 1, True, uniforms(rng, 1, 3, n))
    assert (status == 0).all()
    equal = np.ones((1, n, n))                           # every draw is uniform over the candidates: u = k / m lands ON a boundary
    u = rng.integers(0, 8, size=(1, 3, n - 1)) / 8.0
    check_against_restatement(equal, 0, True, u)
    # infinite entries (algorithms.py:34-36) and all-zero rows (:39-40), without inversion
    Winf = nonmetric(rng, 2, n)
    Winf[rng.random(Winf.shape) < 0.15] = np.inf
    Winf[rng.random(Winf.shape) < 0.05] = -np.inf
    _, status = check_against_restatement(Winf, 0, False, uniforms(rng, 2, 3, n))
    assert (status == 0).all()
    Wzero = nonmetric(rng, 2, n)
    Wzero[0, ::2, :] = 0.0
    Wzero[1, :, :] = 0.0
    Wzero[1, 1, :] = -0.0
    _, status = check_against_restatement(Wzero, 0, False, uniforms(rng, 2, 3, n))
    assert (status == 0).all()


def test_given_u_sixteen_nodes_per_lane():
    """n = 1024: the largest instantiation (16 slots), one walk."""
    rng = np.random.default_rng(5)
    W = make_instance("euclid", 1024, rng)[None]
    _, status = check_against_restatement(W, 1023, True, rng.random((1, 1, 1023)))
    assert (status == 0).all()


# ---- 2. validity ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (3, 64, 100, 257, 600, 1024))
def test_every_tour_is_a_closed_permutation(n):
    rng = np.random.default_rng(n)
    W = nonmetric(rng, 2, n)
    for depot in (0, n - 1):
        for invert in (True, False):
            tours, status = device_walks(W, 6, depot, invert, seed=n + depot)
            assert (status == 0).all() and tours.shape == (2, 6, n + 1)
            assert (tours[:, :, 0] == depot).all() and (tours[:, :, -1] == depot).all()
            assert (np.sort(tours[:, :, :-1], axis=2) == np.arange(n)).all()
    assert len({tuple(t) for t in tours.reshape(-1, n + 1).tolist()}) > 1 or n == 3


# ---- 3. the generator ----------------------------------------------------------------------------------------------------------
def test_generator_is_counter_based():
    rng = np.random.default_rng(3)
    n, B, R, seed = 20, 300, 7, 0x123456789ABCDEF
    W = np.stack([make_instance("euclid", n, rng) for _ in range(B)])
    tours, status = device_walks(W, R, 0, True, seed)
    again, _ = device_walks(W, R, 0, True, seed)
    assert (status == 0).all() and np.array_equal(tours, again)
    other, _ = device_walks(W, R, 0, True, seed + 1)
    assert (other != tours).any(axis=2).mean() > 0.9               # another seed: (nearly) every walk differs
    high, _ = device_walks(W, R, 0, True, seed - (1 << 63))         # bit 63 set (as int64): the key holds all 64 bits of the seed
    assert (high != tours).any(axis=2).mean() > 0.9
    # walk (b, r) alone: its own uniforms, a B = 1, R = 1 launch
    for b, r in ((0, 0), (0, 6), (299, 0), (299, 6), (137, 3)):
        u = philox_uniforms(seed, 1, 1, n - 1, b0=b, r0=r)
        alone, _ = device_walks(W[b:b + 1], 1, 0, True, 0, u)
        assert np.array_equal(alone[0, 0], tours[b, r]), (b, r)
    # ... and in launches of other shapes that contain it
    part, _ = device_walks(W[:138], 4, 0, True, seed)
    assert np.array_equal(part, tours[:138, :4])
    # the whole launch is the restatement under the restated stream
    ref, _ = restated_walks(W[:4], 0, True, philox_uniforms(seed, 4, R, n - 1))
    assert np.array_equal(ref, tours[:4])
    empty, st = device_walks(W[:0], R, 0, True, seed)
    assert empty.shape == (0, R, n + 1) and st.shape == (0, R)


# ---- 4. the law ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("invert", (True, False))
def test_device_walks_follow_the_law(invert):
    z = np.load(LAW_FIXTURE)
    W, depot, calls = z["W"], int(z["depot"]), int(z["calls"])
    tours = all_tours(6, depot)
    index = {tuple(t): k for k, t in enumerate(tours)}
    walks, status = device_walks(W[None], calls, depot, invert, seed=1)
    assert (status == 0).all()
    counts = np.zeros(len(tours))
    for t in walks[0].tolist():
        counts[index[tuple(t)]] += 1
    probs = np.array([tour_probability(W, t, invert) for t in tours])
    stat = chi_square(counts, probs)
    print(f"invert={invert}: chi-square {stat:.1f} (dof 119, bound {chi_square_bound(119):.1f})")
    assert stat < chi_square_bound(119)


# ---- 5. errors -----------------------------------------------------------------------------------------------------------------
def test_bad_weights_stop_only_the_walks_that_meet_them():
    import networkx as nx

    from gnngls_amd import algorithms, ops
    rng = np.random.default_rng(8)
    n, B, R = 20, 2, 16
    W = np.stack([make_instance("euclid", n, rng) for _ in range(B)])
    for bad, invert in ((0.0, True), (np.nan, False), (np.nan, True), (-1.0, False)):
        Wb = W.copy()
        Wb[0, 3, 7] = bad                                # met by the walks of instance 0 that stand on 3 while 7 is unvisited
        u = rng.random((B, R, n - 1))
        tours, status = check_against_restatement(Wb, 0, invert, u)
        hit = status[0] == BAD_WEIGHTS
        assert hit.any() and not hit.all() and (status[1] == 0).all()
        assert (tours[0][hit] == -1).all() and (tours[0][~hit] >= 0).all()
        with pytest.raises(ValueError, match="sample_nn_tours"):
            ops.sample_nn_tours(torch.from_numpy(Wb).cuda(), R, 0, invert, 0, torch.from_numpy(u).cuda())
    G = nx.complete_graph(6)
    for i, j in G.edges:
        G.edges[i, j]["weight"] = 1.0 + i + j
    G.edges[2, 4]["weight"] = 0.0
    with pytest.raises(ValueError):
        algorithms.probabilistic_nearest_neighbour(G, 0, seed=1)
    with pytest.raises(ValueError):
        algorithms.best_probabilistic_nearest_neighbour(G, 0, 4, seed=1)
    assert len(algorithms.probabilistic_nearest_neighbour(G, 0, invert=False, seed=1)) == 7      # a probability of zero is one


# ---- 6. best of R --------------------------------------------------------------------------------------------------------------
def test_best_sampled_tour_is_the_first_strictly_cheapest():
    from gnngls_amd import algorithms, datasets, ops
    from gnngls_amd.algorithms import _attr_matrix
    rng = np.random.default_rng(11)
    n, B, R = 30, 5, 12
    W = torch.from_numpy(np.stack([make_instance("euclid", n, rng) for _ in range(B)])).cuda()
    tours, _ = ops.sample_nn_tours(W, R, 0, True, 21)
    cost = torch.stack([ops.tour_cost(tours[:, r].contiguous(), W) for r in range(R)], dim=1).cpu().numpy()
    best, best_cost = ops.best_sampled_tour(W, W, R, 0, True, 21)
    for b in range(B):
        k = int(np.argmin(cost[b]))                      # np.argmin: the first minimum
        assert best[b].tolist() == tours[b, k].tolist() and best_cost[b].item() == cost[b, k]
    # a constructed tie: under unit costs every tour costs n exactly, so walk 0 is returned
    ones = torch.ones_like(W)
    tie, tie_cost = ops.best_sampled_tour(W, ones, R, 0, True, 21)
    assert torch.equal(tie, tours[:, 0]) and (tie_cost == float(n)).all()
    # the mirror on a reference-format instance
    name = open(os.path.join(FIX, "test.txt")).read().split()[0]
    G = datasets.read_gpickle(os.path.join(FIX, name))
    Wg = ops.as_dev(_attr_matrix(G, "weight")[None], torch.float64)
    expect, _ = ops.best_sampled_tour(Wg, Wg, 16, 0, True, 3)
    got = algorithms.best_probabilistic_nearest_neighbour(G, 0, 16, seed=3)
    assert got == expect[0].tolist() and sorted(got[:-1]) == list(range(12)) and got[0] == got[-1] == 0
    one = algorithms.probabilistic_nearest_neighbour(G, 0, seed=3)
    assert one == ops.sample_nn_tours(Wg, 1, 0, True, 3)[0][0, 0].tolist()
    np.random.seed(4)
    a = algorithms.probabilistic_nearest_neighbour(G, 0)
    np.random.seed(4)
    assert algorithms.probabilistic_nearest_neighbour(G, 0) == a               # seed=None: repeatable under np.random.seed


# ---- 7. multi-start ------------------------------------------------------------------------------------------------------------
TENSOR_FIELDS = ("best_tour", "best_cost", "init_cost", "outer_iters", "evals", "moves", "status")


def same_results(a, b):
    for f in TENSOR_FIELDS + ("start_costs", "best_start"):
        x, y = getattr(a, f), getattr(b, f)
        assert (x is None) == (y is None), f
        if x is not None:
            assert torch.equal(x, y), f


def test_multi_start_search():
    from gnngls_amd import ops, pipeline
    from gnngls_amd.synthetic import random_instances
    D = torch.from_numpy(random_instances(np.random.default_rng(2), 4, 20)[0]).cuda()
    kw = dict(guides=("weight",), max_outer_iters=3)
    base = pipeline.solve_batch(D, **kw)
    one = pipeline.solve_batch(D, starts=1, **kw)
    same_results(base, one)
    for f in ("regret_pred", "trace_cost", "trace_time", "imp_cost", "imp_time", "imp_iter", "imp_len", "evals_executed",
              "lower_bound", "bound_exit", "start_costs", "best_start"):
        assert getattr(one, f) is None and getattr(base, f) is None, f
    assert set(one.timing) == set(base.timing) and one.timing["chunks"] == base.timing["chunks"] == 1
    assert one.start_time.shape == base.start_time.shape and one.launch_time.shape == base.launch_time.shape

    r = pipeline.solve_batch(D, starts=4, start_seed=5, **kw)
    assert r.start_costs.shape == (4, 4) and r.start_costs.dtype == torch.float64 and r.best_start.shape == (4,)
    assert torch.equal(r.start_costs[:, 0], base.best_cost)                   # run 0 is the single-start search, bit for bit
    assert torch.equal(r.best_cost, r.start_costs.min(dim=1).values)
    sc = r.start_costs.cpu().numpy()
    assert r.best_start.cpu().tolist() == [int(np.argmin(row)) for row in sc]  # the first arg-min
    # best_cost is the reference's running sum (algorithms.py:143,175: the start tour's cost plus the delta of every accepted
    # move), not a recomputed length: the two differ by rounding only.  n adds in tour_cost, and per accepted move one add and a
    # delta of at most 7 operations, each rounded to 2^-53 of a magnitude below twice the start tour's cost
    err = (ops.tour_cost(r.best_tour, D) - r.best_cost).abs()
    bound = (20 + 8 * (r.moves.double() + 1)) * 2.0 ** -53 * 2.0 * r.init_cost
    print("length of best_tour against best_cost:", err.tolist(), "bound", bound.tolist())
    assert (err <= bound).all()
    assert (r.best_cost <= base.best_cost).all() and "sample_s" in r.timing and r.timing["sample_s"] >= 0.0
    assert r.best_tour.shape == (4, 21) and r.status.shape == (4,) and r.outer_iters.tolist() == [3] * 4
    same_results(r, pipeline.solve_batch(D, starts=4, start_seed=5, **kw))
    other = pipeline.solve_batch(D, starts=4, start_seed=6, **kw)
    assert torch.equal(other.start_costs[:, 0], r.start_costs[:, 0]) and not torch.equal(other.start_costs, r.start_costs)
    # with the measurement hooks: the winner's rows
    h = pipeline.solve_batch(D, starts=4, start_seed=5, imp_cap=8, lower_bound=True, **kw)
    same_results(r, h)
    assert h.imp_cost.shape == (4, 8) and h.lower_bound.shape == (4,) and (h.lower_bound <= h.best_cost * (1 + 1e-12)).all()
    empty = pipeline.solve_batch(D[:0], starts=4, **kw)
    assert empty.start_costs.shape == (0, 4) and empty.best_start.shape == (0,)


def test_multi_start_chunks():
    """R > capacity // B: the batch is cut into chunks of capacity // R instances; the sampled starts belong to the instance,
    so any chunking gives the same result."""
    from gnngls_amd import ops, pipeline
    from gnngls_amd.synthetic import random_instances
    n, B = 100, 4
    cap = ops.gls_resident_capacity(n)
    R = cap // B + 44
    assert cap // R < B
    D = torch.from_numpy(random_instances(np.random.default_rng(9), B, n)[0]).cuda()
    kw = dict(guides=("weight",), max_outer_iters=2, starts=R, start_seed=1)
    auto = pipeline.solve_batch(D, **kw)
    assert auto.timing["chunks"] == -(-B // (cap // R)) > 1
    forced = pipeline.solve_batch(D, chunk=1, **kw)
    assert forced.timing["chunks"] == B
    same_results(auto, forced)
    assert torch.equal(auto.best_cost, auto.start_costs.min(dim=1).values)


# ---- 8. the command line -------------------------------------------------------------------------------------------------------
def test_cli_with_starts(tmp_path):
    data = tmp_path / "tsp12"
    shutil.copytree(FIX, data)
    mdir = tmp_path / "models" / "tsp12"
    mdir.mkdir(parents=True)
    json.dump({"embed_dim": 128, "n_layers": 3, "n_heads": 8}, open(mdir / "params.json", "w"))
    run_dir = tmp_path / "runs"
    subprocess.check_call([sys.executable, os.path.join(ROOT, "scripts", "test.py"), str(data / "test.txt"),
                           str(mdir / "checkpoint_best_val.pt"), str(run_dir), "weight", "--time_limit", "0.3", "--starts", "4"],
                          cwd=ROOT)
    df = pickle.load(open(next(run_dir.glob("*.pkl")), "rb"))
    assert sorted(df.columns) == sorted(["instance", "time", "opt_cost", "cost", "best_cost", "gap", "dt"])
    names = open(os.path.join(FIX, "test.txt")).read().split()
    assert sorted(df["instance"].unique()) == sorted(names)
    last = df.groupby("instance")["gap"].last()
    assert (last >= -1e-7).all()
