"""GPU checks of alpha-nearness (gnngls_alpha_nearness, alpha_kernels.hip) against the NumPy restatement of its definition,
gnngls_amd.host.alpha_nearness (itself pinned to a tree-free closure in tests/test_alpha_cpu.py): equality always means equal
bit patterns of every entry.  Instances are euclid(default_rng(1000 + n), n) as in the bound's tests.  Then the plumbing: the
guide reaches the search kernel unchanged through solve_batch, the single-graph mirror and the command line."""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

from gnngls_amd import host  # noqa: E402
from test_alpha_cpu import bits, tie_heavy  # noqa: E402
from test_one_tree_cpu import euclid  # noqa: E402

# the layout's edges: one wavefront with 1, 2, 3, 4 nodes per lane (64 / 65, 128 / 129, 192 / 193, 256), then 2, 3, 4 wavefronts
SIZES = [(n, 3) for n in (3, 4, 5, 8, 20, 64, 65, 128, 129, 192, 193, 256, 257)] + [(513, 1), (1024, 1)]


def dev(x, dtype=torch.float64):
    from gnngls_amd import ops
    return ops.as_dev(np.asarray(x), dtype)


def instances(n, count):
    rng = np.random.default_rng(1000 + n)
    return np.stack([euclid(rng, n) for _ in range(count)])


def nn_length(D):
    from gnngls_amd import ops
    return ops.tour_cost(ops.nearest_neighbor(D), D)


def assert_same(got, Ds, pis, what):
    got = got.cpu().numpy()
    for b, D in enumerate(Ds):
        want = host.alpha_nearness(D, None if pis is None else pis[b])
        same = bits(got[b]) == bits(want)
        assert same.all(), (what, b, int((~same).sum()), np.argwhere(~same)[:4].tolist(), float(np.nanmax(np.abs(got[b] - want))))


@pytest.mark.parametrize("n,count", SIZES)
def test_sizes_equal_the_host_reference(n, count):
    from gnngls_amd import ops
    Ds = instances(n, count)
    D = dev(Ds)
    assert_same(ops.alpha_nearness(D), Ds, None, f"n={n} pi=None")
    r = ops.one_tree_bound(D, nn_length(D), max_iters=100 if n <= 257 else 20)
    assert_same(ops.alpha_nearness(D, r.pi), Ds, r.pi.cpu().numpy(), f"n={n} pi of the ascent")
    pis = np.random.default_rng(5000 + n).normal(scale=0.1, size=(count, n))
    a = ops.alpha_nearness(D, dev(pis))
    assert_same(a, Ds, pis, f"n={n} random pi")
    assert torch.equal(a, a.transpose(1, 2)) and bool((a >= 0).all()) and bool((a.diagonal(dim1=1, dim2=2) == 0).all())


@pytest.mark.parametrize("n", [20, 100])
def test_tie_heavy_integer_matrix(n):
    from gnngls_amd import ops
    rng = np.random.default_rng(2000 + n)
    Ds = np.stack([tie_heavy(rng, n) for _ in range(3)])
    pis = rng.integers(-2, 3, size=(3, n)).astype(float)
    assert_same(ops.alpha_nearness(dev(Ds)), Ds, None, f"ties n={n} pi=None")
    assert_same(ops.alpha_nearness(dev(Ds), dev(pis)), Ds, pis, f"ties n={n} integer pi")


def test_batch_independence():
    from gnngls_amd import ops
    Ds = instances(50, 5)
    pis = np.random.default_rng(50).normal(scale=0.1, size=(5, 50))
    batch = ops.alpha_nearness(dev(Ds), dev(pis))
    alone = ops.alpha_nearness(dev(Ds[2:3]), dev(pis[2:3]))
    assert torch.equal(batch[2:3], alone)
    assert_same(alone, Ds[2:3], pis[2:3], "n=50 alone")


def test_asymmetric_matrix_is_flagged():
    from gnngls_amd import _lib, ops
    Ds = instances(20, 4).copy()
    Ds[2, 7, 11] = np.nextafter(Ds[2, 7, 11], np.inf)  # one ulp in one triangle
    D = dev(Ds)
    with pytest.raises(ValueError, match=r"instances \[2\].*symmetric"):
        ops.alpha_nearness(D)
    out = torch.full((4, 20, 20), -7.0, dtype=torch.float64, device="cuda")
    status = torch.full((4,), -7, dtype=torch.int32, device="cuda")
    assert _lib.load().gnngls_alpha_nearness(_lib.ptr(D), None, 4, 20, _lib.ptr(out), _lib.ptr(status), _lib.current_stream()) == 0
    torch.cuda.synchronize()
    assert status.tolist() == [0, 0, ops.STATUS_ASYMMETRIC, 0]
    assert bool(torch.isnan(out[2]).all())
    ok = [0, 1, 3]
    assert_same(out[ok], Ds[ok], None, "the symmetric instances of the batch")


def test_torch_op():
    import gnngls_amd.torch_ops  # noqa: F401
    from gnngls_amd import ops
    D = dev(instances(12, 4))
    pi = ops.one_tree_bound(D, nn_length(D), max_iters=200).pi
    assert torch.equal(torch.ops.gnngls.alpha_nearness(D, pi), ops.alpha_nearness(D, pi))
    assert torch.equal(torch.ops.gnngls.alpha_nearness(D, None), ops.alpha_nearness(D))


def test_guide_reaches_the_search_unchanged():
    """solve_batch with guides ('alpha', 'weight') == ops.gls_run on the guide tensor built by hand == the oracle's search fed
    the host reference's alpha of the device's pi.  The search kernel is bit-exact with the oracle for any guide matrix, so a
    difference is a plumbing fault."""
    from gnngls_amd import ops, pipeline
    from oracle import gls_oracle
    Ds = instances(20, 4)
    D = dev(Ds)
    res = pipeline.solve_batch(D, guides=("alpha", "weight"), max_outer_iters=5, perturbation_moves=20)
    assert res.timing["alpha_s"] > 0
    assert "alpha_s" not in pipeline.solve_batch(D, guides=("weight",), max_outer_iters=1).timing

    pi = ops.one_tree_bound(D, nn_length(D), max_iters=2000).pi
    A = ops.alpha_nearness(D, pi)
    init = ops.nearest_neighbor(D)
    init_cost = ops.tour_cost(init, D)
    r = ops.gls_run(D, torch.stack([A, D]).contiguous(), init, init_cost, perturbation_moves=20, max_outer_iters=5)
    assert torch.equal(res.best_tour, r.best_tour) and torch.equal(res.best_cost, r.best_cost)

    pis = pi.cpu().numpy()
    for b in range(4):
        g = np.stack([host.alpha_nearness(Ds[b], pis[b]), Ds[b]])
        o = gls_oracle.guided_local_search(Ds[b], g, init[b].tolist(), float(init_cost[b]), perturbation_moves=20, max_outer_iters=5)
        assert o["best_tour"] == res.best_tour[b].tolist(), b
        assert bits(o["best_cost"]) == bits(float(res.best_cost[b])), b

    # any order and mix; alpha_iters = 0 takes zero potentials; other names are still refused
    z = pipeline.solve_batch(D, guides=("weight", "alpha"), max_outer_iters=2, alpha_iters=0)
    rz = ops.gls_run(D, torch.stack([D, ops.alpha_nearness(D)]).contiguous(), init, init_cost, perturbation_moves=20, max_outer_iters=2)
    assert torch.equal(z.best_tour, rz.best_tour) and torch.equal(z.best_cost, rz.best_cost)
    with pytest.raises(ValueError, match="unknown guide"):
        pipeline.solve_batch(D, guides=("alpha", "beta"), max_outer_iters=1)


def test_multi_start_replicates_the_alpha_matrices():
    from gnngls_amd import pipeline
    D = dev(instances(20, 3))
    one = pipeline.solve_batch(D, guides=("alpha",), max_outer_iters=3)
    many = pipeline.solve_batch(D, guides=("alpha",), max_outer_iters=3, starts=3)
    assert torch.equal(many.start_costs[:, 0], one.best_cost)          # run 0 is the single-start search
    assert bool((many.best_cost <= one.best_cost).all())


def test_single_graph_mirror():
    import time
    import gnngls_amd
    from gnngls_amd import algorithms, datasets, ops
    from gnngls_amd.algorithms import _attr_matrix
    from test_n3_ingestion_cpu import names
    G = datasets.read_gpickle(os.path.join(ROOT, "tests", "golden", "n3_tsp12", names()[0]))
    assert algorithms.alpha_nearness(G) is G
    D = dev(_attr_matrix(G, "weight")[None])
    A = ops.alpha_nearness(D, ops.one_tree_bound(D, nn_length(D), max_iters=2000).pi)[0].cpu().numpy()
    assert all(bits(G.edges[u, v]["alpha"]) == bits(A[u, v]) for u, v in G.edges)
    init = algorithms.nearest_neighbor(G, 0)
    tour, cost, progress = algorithms.guided_local_search(G, init, gnngls_amd.tour_cost(G, init), time.time() + 10, guides=["alpha"],
                                                          perturbation_moves=5, max_outer_iters=3)
    assert gnngls_amd.is_valid_tour(G, tour) and len(progress) >= 0
    assert abs(cost - gnngls_amd.tour_cost(G, tour)) <= 1e-9 * cost and cost <= gnngls_amd.tour_cost(G, init) * (1 + 1e-9)


def test_cli_alpha_guide(tmp_path):
    fix = os.path.join(ROOT, "tests", "golden", "n3_tsp12")
    data = tmp_path / "tsp12"
    shutil.copytree(fix, data)
    mdir = tmp_path / "models" / "tsp12"
    mdir.mkdir(parents=True)
    json.dump({"embed_dim": 128, "n_layers": 3, "n_heads": 8}, open(mdir / "params.json", "w"))
    run_dir = tmp_path / "runs"
    subprocess.check_call([sys.executable, os.path.join(ROOT, "scripts", "test.py"), str(data / "test.txt"),
                           str(mdir / "checkpoint_best_val.pt"), str(run_dir), "alpha", "--time_limit", "0.2", "--use_gpu",
                           "--alpha_iters", "500"], cwd=ROOT)
    df = pickle.load(open(next(run_dir.glob("*.pkl")), "rb"))
    assert list(df.columns) == ["instance", "time", "opt_cost", "cost", "best_cost", "gap", "dt"]
    assert (df.groupby("instance")["gap"].last() >= -1e-7).all()
