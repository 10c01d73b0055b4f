"""GPU checks of the insertion tour constructors (reference algorithms.py:67-108): every comparison is bit-exact -- tours as
integer lists, costs by ==.  The oracle of the fuzz is the NumPy restatement of tests/test_insertion_cpu.py, which that file
pins to fixtures captured from the reference."""
import ctypes
import json
import os
import pickle
import shutil
import subprocess
import sys

import networkx as nx
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from test_insertion_cpu import (KINDS, MODES, insertion_cases, make_instance, restated_cheapest_insertion,  # noqa: E402
                                restated_insertion, step_cases)


def dev(D):
    from gnngls_amd import ops
    return ops.as_dev(np.asarray(D, dtype=np.float64), torch.float64)


def graph_of(D):
    G = nx.complete_graph(D.shape[0])
    for i, j in G.edges:
        G.edges[i, j]["weight"] = D[i, j]
    return G


@pytest.mark.parametrize("route", ["ops", "algorithms", "torch_ops"])
def test_fixtures_reproduced(route):
    import gnngls_amd.torch_ops  # noqa: F401
    from gnngls_amd import algorithms, ops
    for c in insertion_cases():
        D, depot, mode = c["D"], c["depot"], c["mode"]
        if mode == "random":
            np.random.seed(c["seed"])
        if route == "ops":
            tour = ops.insertion(dev(D[None]), depot, mode)[0].tolist()
        elif route == "algorithms":
            tour = algorithms.insertion(graph_of(D), depot, mode=mode)
            assert type(tour) is list
        else:
            tour = torch.ops.gnngls.insertion(dev(D[None]), depot, mode, None)[0].tolist()
        assert tour == c["tour"], (route, c["id"])
        if mode == "random":
            assert np.random.random() == c["next_draw"], (route, c["id"])      # NumPy's stream is where the reference leaves it
    for s in step_cases():
        D = s["D"]
        sub = ops.as_dev(np.asarray(s["sub_tour"], dtype=np.int32)[None], torch.int32)
        node = ops.as_dev(np.asarray([s["node"]], dtype=np.int32), torch.int32)
        if route == "ops":
            t, cost = ops.cheapest_insertion(sub, node, dev(D[None]))
            assert t[0].tolist() == s["tour"] and cost[0].item() == s["cost"], s["id"]
        elif route == "algorithms":
            assert algorithms.cheapest_insertion(graph_of(D), list(s["sub_tour"]), s["node"]) == s["tour"], s["id"]
        else:
            t, cost = torch.ops.gnngls.cheapest_insertion(sub, node, dev(D[None]))
            assert t[0].tolist() == s["tour"] and cost[0].item() == s["cost"], s["id"]


def test_seeded_fuzz_against_the_restatement():
    """n in 2..260 (2, 3, 200 and 257 forced) plus one n = 500 instance, every instance kind, every mode, batches of 1..64
    (1..8 from n = 100 on, to bound the host time of the restatement), random depots.  No case is skipped or filtered: the
    tolerated share of mismatches is 0."""
    from gnngls_amd import ops
    rng = np.random.default_rng(777)
    sizes = [2, 3, 200, 257] + [int(x) for x in rng.integers(2, 261, size=56)]
    plan = [(n, KINDS[k % 4], MODES[(k // 4) % 3], int(rng.integers(1, 65 if n < 100 else 9))) for k, n in enumerate(sizes)]
    plan.append((500, "euclid", "farthest", 1))
    assert {(kind, mode) for _, kind, mode, _ in plan} == {(k, m) for k in KINDS for m in MODES}
    checked = 0
    for case, (n, kind, mode, B) in enumerate(plan):
        Ds = np.stack([make_instance(kind, n, rng) for _ in range(B)])
        depot = int(rng.integers(0, n))
        np.random.seed(1000 + case)
        got = ops.insertion(dev(Ds), depot, mode).cpu().tolist()
        after = np.random.random()
        np.random.seed(1000 + case)
        want = [restated_insertion(Ds[b], depot, mode) for b in range(B)]
        assert np.random.random() == after, (case, n, kind, mode)
        for b in range(B):
            assert got[b] == want[b], (case, n, kind, mode, B, depot, b)
            checked += 1
    assert checked == sum(p[3] for p in plan)


def test_wide_workgroups():
    """n = 1100 runs on 9 wavefronts (both stages of the workgroup arg-min) with a tie-heavy matrix; n = 2048 is the largest
    supported instance (16 wavefronts, 98 KiB of LDS): a valid tour from the depot."""
    from gnngls_amd import ops
    D = make_instance("grid", 1100, np.random.default_rng(41))
    assert ops.insertion(dev(D[None]), 613, "nearest")[0].tolist() == restated_insertion(D, 613, "nearest")
    D = make_instance("euclid", ops.INSERTION_MAX_N, np.random.default_rng(42))
    t = ops.insertion(dev(D[None]), 7, "farthest")[0].tolist()
    assert t[0] == t[-1] == 7 and sorted(t[:-1]) == list(range(ops.INSERTION_MAX_N))


def test_cheapest_insertion_fuzz():
    from gnngls_amd import ops
    rng = np.random.default_rng(778)
    for case in range(40):
        n = int(rng.integers(2, 261))
        kind = KINDS[case % 4]
        B = int(rng.integers(1, 33))
        ln = int(rng.integers(2, n + 1))                     # entries of the closed sub-tour: 2 .. n
        Ds = np.stack([make_instance(kind, n, rng) for _ in range(B)])
        subs, nodes = [], []
        for b in range(B):
            perm = rng.permutation(n)
            subs.append([perm[0]] + perm[1:ln - 1].tolist() + [perm[0]])
            nodes.append(perm[ln - 1])
        t, cost = ops.cheapest_insertion(ops.as_dev(np.asarray(subs, dtype=np.int32), torch.int32),
                                         ops.as_dev(np.asarray(nodes, dtype=np.int32), torch.int32), dev(Ds))
        t, cost = t.cpu().tolist(), cost.cpu().tolist()
        for b in range(B):
            wt, wc = restated_cheapest_insertion(Ds[b], subs[b], nodes[b])
            assert t[b] == wt and cost[b] == wc, (case, n, kind, ln, b)


def test_batch_of_1024_equals_one_instance_per_call():
    from gnngls_amd import ops
    rng = np.random.default_rng(5)
    pos = rng.random((1024, 100, 2))
    D = dev(np.linalg.norm(pos[:, :, None, :] - pos[:, None, :, :], axis=-1))
    for mode in ("nearest", "farthest"):
        full = ops.insertion(D, 0, mode)
        assert full.shape == (1024, 101)
        for b in rng.choice(1024, size=32, replace=False).tolist():
            one = ops.insertion(D[b:b + 1].contiguous(), 0, mode)
            assert torch.equal(one[0], full[b]), (mode, b)
            assert sorted(full[b, :-1].tolist()) == list(range(100))


def test_bad_order_rows_are_reported_and_left_untouched():
    from gnngls_amd import _lib, ops
    rng = np.random.default_rng(6)
    B, n, depot = 6, 12, 3
    Ds = np.stack([make_instance("euclid", n, rng) for _ in range(B)])
    good = [[int(x) for x in rng.permutation([j for j in range(n) if j != depot])] for _ in range(B)]
    order = [list(r) for r in good]
    order[1][4] = order[1][7]            # a repeated node
    order[3][0] = depot                  # the depot
    order[4][10] = n                     # an id >= n
    order[5][2] = -1                     # a negative id
    W = dev(Ds)
    o = ops.as_dev(np.asarray(order, dtype=np.int32), torch.int32)
    out = torch.full((B, n + 1), -7, dtype=torch.int32, device=W.device)
    status = torch.full((B,), -1, dtype=torch.int32, device=W.device)
    code = _lib.load().gnngls_insertion(_lib.ptr(W), B, n, depot, ops.INSERT_MODES["random"], _lib.ptr(o), _lib.ptr(out),
                                        _lib.ptr(status), _lib.current_stream())
    assert code == 0
    torch.cuda.synchronize()
    assert status.tolist() == [0, ops.STATUS_BAD_ORDER, 0, ops.STATUS_BAD_ORDER, ops.STATUS_BAD_ORDER, ops.STATUS_BAD_ORDER]
    for b in range(B):
        if b in (0, 2):
            assert out[b].tolist() == restated_insertion(Ds[b], depot, "random", order=good[b]), b
        else:
            assert out[b].tolist() == [-7] * (n + 1), b
    with pytest.raises(ValueError, match="not permutations"):
        ops.insertion(W, depot, "random", order=o)
    assert ops.insertion(W, depot, "random", order=ops.as_dev(np.asarray(good, dtype=np.int32), torch.int32))[0].tolist() == \
        restated_insertion(Ds[0], depot, "random", order=good[0])


def test_small_sizes_and_limits():
    from gnngls_amd import _lib, ops
    assert ops.insertion(dev(np.zeros((2, 1, 1))), 0, "farthest").tolist() == [[0, 0], [0, 0]]
    assert ops.insertion(dev(np.zeros((1, 1, 1))), 0, "random").tolist() == [[0, 0]]
    D2 = np.array([[[0.0, 2.0], [2.0, 0.0]]])
    for mode in MODES:
        assert ops.insertion(dev(D2), 1, mode).tolist() == [[1, 0, 1]]
    with pytest.raises(_lib.GnnglsHipError, match="n=2049"):
        ops.insertion(torch.zeros((1, 2049, 2049), dtype=torch.float64, device="cuda"), 0, "nearest")
    # an index out of range in a sub-tour: refused, nothing read out of range
    with pytest.raises(ValueError, match="out of 0..n-1"):
        ops.cheapest_insertion(ops.as_dev(np.asarray([[0, 9, 0]], dtype=np.int32), torch.int32),
                               ops.as_dev(np.asarray([1], dtype=np.int32), torch.int32), dev(np.zeros((1, 4, 4))))


def test_profile_kind():
    from gnngls_amd import _lib, ops
    D = dev(make_instance("euclid", 20, np.random.default_rng(1))[None])
    _lib.profile_enable(True)
    try:
        ops.insertion(D, 0, "nearest")
        ops.nearest_neighbor(D)
        prof = _lib.profile_collect()
    finally:
        _lib.profile_enable(False)
    assert prof["insertion"][1] == 1 and prof["insertion"][0] > 0.0 and prof["nearest_neighbor"][1] == 1


def test_solve_batch_start_tours():
    from gnngls_amd import ops, pipeline
    rng = np.random.default_rng(9)
    pos = rng.random((8, 50, 2))
    D = dev(np.linalg.norm(pos[:, :, None, :] - pos[:, None, :, :], axis=-1))
    kw = dict(guides=("weight",), max_outer_iters=6, perturbation_moves=20)
    a = pipeline.solve_batch(D, **kw)
    b = pipeline.solve_batch(D, init="nearest_neighbor", init_weight="auto", **kw)
    for name in ("best_tour", "best_cost", "init_cost", "outer_iters", "evals", "moves", "status"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert torch.equal(a.init_cost, ops.tour_cost(ops.nearest_neighbor(D), D))
    for init, mode in (("farthest_insertion", "farthest"), ("nearest_insertion", "nearest")):
        r = pipeline.solve_batch(D, init=init, **kw)
        assert torch.equal(r.init_cost, ops.tour_cost(ops.insertion(D, 0, mode), D)), init
        assert bool((r.best_cost <= r.init_cost).all()), init
        assert bool((r.status == 0).all())
    with pytest.raises(ValueError, match="unknown start tour"):
        pipeline.solve_batch(D, init="cheapest", **kw)
    with pytest.raises(ValueError, match="unknown init_weight"):
        pipeline.solve_batch(D, init_weight="regret", **kw)
    # with the model as guide: "auto" builds the start on regret_pred (the reference's rule), "weight" on the distances
    model = pipeline.synthetic_model()
    sc = pipeline.Scalers.fit_weights(D)
    kw = dict(guides=("regret_pred",), max_outer_iters=3, perturbation_moves=20, keep_regret=True)
    r = pipeline.solve_batch(D, model, sc, init="farthest_insertion", **kw)
    assert torch.equal(r.init_cost, ops.tour_cost(ops.insertion(r.regret_pred, 0, "farthest"), D))
    r = pipeline.solve_batch(D, model, sc, init="farthest_insertion", init_weight="weight", **kw)
    assert torch.equal(r.init_cost, ops.tour_cost(ops.insertion(D, 0, "farthest"), D))
    r0 = pipeline.solve_batch(D, model, sc, **kw)
    assert torch.equal(r0.init_cost, ops.tour_cost(ops.nearest_neighbor(r0.regret_pred), D))


def test_cli_with_farthest_insertion_start(tmp_path):
    from test_n3_ingestion_cpu import dgl061_checkpoint, names
    fix = os.path.join(ROOT, "tests", "golden", "n3_tsp12")
    data = tmp_path / "tsp12"
    shutil.copytree(fix, data)
    mdir = tmp_path / "models" / "tsp12"
    mdir.mkdir(parents=True)
    torch.save(dgl061_checkpoint(), mdir / "checkpoint_best_val.pt")
    json.dump({"embed_dim": 128, "n_layers": 3, "n_heads": 8}, open(mdir / "params.json", "w"))
    for extra in ([], ["--init_weight", "weight"]):
        run_dir = tmp_path / ("runs" + "_".join(extra).replace("-", ""))
        subprocess.check_call([sys.executable, os.path.join(ROOT, "scripts", "test.py"), str(data / "test.txt"),
                               str(mdir / "checkpoint_best_val.pt"), str(run_dir), "regret_pred", "--time_limit", "0.3",
                               "--use_gpu", "--init_tour", "farthest_insertion"] + extra, cwd=ROOT)
        df = pickle.load(open(next(run_dir.glob("*.pkl")), "rb"))
        assert sorted(df["instance"].unique()) == sorted(names())
        g = df.groupby("instance")
        # every instance's record ends on its returned cost: the last best_cost is the minimum of its cost rows, and the
        # search closes TSP12 from this start as it does from nearest neighbour
        assert (g["best_cost"].last() == g["cost"].min()).all()
        assert np.allclose(g["opt_cost"].first().to_numpy(), g["best_cost"].last().to_numpy(), rtol=1e-12)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "test.py"), str(data / "test.txt"),
                        str(mdir / "checkpoint_best_val.pt"), str(tmp_path / "x"), "weight", "--init_tour", "cheapest"],
                       cwd=ROOT, capture_output=True, text=True)
    assert p.returncode != 0 and "--init_tour" in p.stderr


def test_ctypes_entry_matches_header_signature():
    """The raw entry with explicit ctypes arguments (what a C caller does): mode constants of the header."""
    from gnngls_amd import _lib
    D = make_instance("grid", 30, np.random.default_rng(2))
    W = dev(D[None])
    out = torch.zeros((1, 31), dtype=torch.int32, device=W.device)
    L = _lib.load()
    for code, mode in ((0, "nearest"), (1, "farthest")):
        assert L.gnngls_insertion(_lib.ptr(W), 1, 30, 7, code, None, _lib.ptr(out), None, _lib.current_stream()) == 0
        torch.cuda.synchronize()
        assert out[0].tolist() == restated_insertion(D, 7, mode)
    assert L.gnngls_insertion(_lib.ptr(W), 1, 30, 7, 2, None, _lib.ptr(out), None, ctypes.c_void_p(0)) == -1
