"""GPU checks of the Held-Karp 1-tree bound (gnngls_one_tree_bound, bounds_kernels.hip) against its definition, oracle/one_tree.c:
equality always means equal bit patterns of the bound.  Instances are euclid(default_rng(1000 + n), n) as in
tests/test_one_tree_cpu.py; device and oracle receive the same double ub (the nearest-neighbour tour's length unless stated)."""
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

from oracle import held_karp as hk  # noqa: E402
from oracle import one_tree as ot  # noqa: E402
from test_one_tree_cpu import euclid  # noqa: E402

SIZES = (3, 4, 5, 8, 12, 20, 49, 50, 64, 65, 100, 129, 200)


def dev(x, dtype=torch.float64):
    from gnngls_amd import ops
    return ops.as_dev(np.asarray(x), dtype)


def bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def instances(n, count=None):
    rng = np.random.default_rng(1000 + n)
    return np.stack([euclid(rng, n) for _ in range(count or (6 if n <= 65 else 3))])


def nn_length(D):
    from gnngls_amd import ops
    return ops.tour_cost(ops.nearest_neighbor(D), D)


def device_bound(Ds, ub=None, max_iters=2000, want_pi=True):
    """Ds [B,n,n] host -> (OneTreeResult, ub as host doubles)."""
    from gnngls_amd import ops
    D = dev(Ds)
    ub = nn_length(D) if ub is None else dev(ub)
    r = ops.one_tree_bound(D, ub, max_iters=max_iters, want_pi=want_pi)
    torch.cuda.synchronize()
    return r, ub.cpu().numpy()


def oracle_bounds(Ds, ub, max_iters=2000):
    return np.array([ot.lower_bound(D, float(u), max_iters) for D, u in zip(Ds, ub)])


def assert_same(r, Ds, ub, max_iters=2000, what=""):
    want = oracle_bounds(Ds, ub, max_iters)
    got = r.bound.cpu().numpy()
    print(what, "device", got.tolist(), "oracle", want.tolist())
    assert np.array_equal(bits(got), bits(want)), (what, got.tolist(), want.tolist())
    assert bool((r.status == 0).all())


def one_tree_value(c, pi):
    """NumPy restatement of min_one_tree (oracle/one_tree.c:23-46) and of w(pi) (one_tree.c:60-62): Prim on nodes 1..n-1 with a
    sequential `total`, the candidate weights vectorised as (cu + pi[u]) + pi."""
    n = c.shape[0]
    deg = np.zeros(n, dtype=np.int64)
    inside = np.zeros(n, dtype=bool)
    inside[0] = True                                   # node 0 never takes part in Prim
    key = np.full(n, np.finfo(np.float64).max)
    parent = np.full(n, -1)
    key[1] = 0.0
    total = 0.0
    for _ in range(1, n):
        u = int(np.argmin(np.where(inside, np.inf, key)))          # first strictly smallest key
        inside[u] = True
        if parent[u] >= 0:
            total += key[u]; deg[u] += 1; deg[parent[u]] += 1
        w = (c[u] + pi[u]) + pi
        upd = ~inside & (w < key)
        key[upd] = w[upd]; parent[upd] = u
    w0 = (c[0] + pi[0]) + pi
    order = sorted(range(1, n), key=lambda v: (w0[v], v))          # the two lexicographically smallest (weight, node)
    total += w0[order[0]] + w0[order[1]]
    deg[0] = 2; deg[order[0]] += 1; deg[order[1]] += 1
    sum_pi = 0.0
    for x in pi:
        sum_pi += x
    return total - 2.0 * sum_pi, deg


# ---- 1. sizes ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sweep():
    out = {}
    for n in SIZES:
        Ds = instances(n)
        r, ub = device_bound(Ds)
        out[n] = (Ds, ub, r)
    return out


@pytest.mark.parametrize("n", SIZES)
def test_sizes_equal_the_oracle(sweep, n):
    Ds, ub, r = sweep[n]
    assert_same(r, Ds, ub, what=f"n={n}")
    iters, kind = r.iters.cpu().numpy(), r.exit_kind.cpu().numpy()
    assert ((iters >= 1) & (iters <= 2000)).all()
    assert ((kind != 0) | (iters == 2000)).all()       # the iteration limit means exactly max_iters 1-trees


def test_sweep_shows_all_three_exits(sweep):
    from gnngls_amd import ops
    kinds = {n: sweep[n][2].exit_kind.cpu().tolist() for n in SIZES}
    print(kinds)
    seen = {k for ks in kinds.values() for k in ks}
    assert seen == {ops.BOUND_EXIT_ITERS, ops.BOUND_EXIT_STEP, ops.BOUND_EXIT_TOUR}, kinds
    # what an instrumented copy of the oracle reported for these seeds
    for n in (3, 4, 5, 8, 12):
        assert set(kinds[n]) == {ops.BOUND_EXIT_TOUR}, (n, kinds[n])
    for n in (49, 100):
        assert set(kinds[n]) == {ops.BOUND_EXIT_STEP}, (n, kinds[n])
    assert set(kinds[200]) == {ops.BOUND_EXIT_ITERS}, kinds[200]


# ---- 2. trajectory -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [8, 20, 100])
def test_trajectory(n):
    Ds = instances(n, 3)
    for max_iters in (1, 2, 3, 7, 26, 27, 60, 300):    # 26 / 27: the first possible halving and restore at period 25
        r, ub = device_bound(Ds, max_iters=max_iters)
        assert_same(r, Ds, ub, max_iters, what=f"n={n} max_iters={max_iters}")
        assert bool((r.iters >= 1).all()) and bool((r.iters <= max_iters).all())


# ---- 3. step rule ------------------------------------------------------------------------------------------------------------
def test_step_rule():
    Ds = instances(20)
    r0, nn = device_bound(Ds)
    lb = r0.bound.cpu().numpy()
    for what, ub in (("1.0 nn", nn), ("1.3 nn", 1.3 * nn), ("10 nn", 10.0 * nn), ("0.5 bound", 0.5 * lb),
                     ("0", np.zeros_like(nn)), ("-1", -np.ones_like(nn))):       # the last three: the fall-back gap
        r, u = device_bound(Ds, ub=ub)
        assert_same(r, Ds, u, what=f"ub={what}")


# ---- 4. ties and non-metric costs --------------------------------------------------------------------------------------------
def lattice(rng, n):
    pos = rng.integers(0, 4, size=(n, 2)).astype(float)
    L = np.abs(pos[:, None] - pos[None]).sum(-1) + 1.0
    np.fill_diagonal(L, 0.0)
    return L


def non_metric(rng, n):
    D = np.triu(rng.random((n, n)), 1)
    return D + D.T


@pytest.mark.parametrize("kind,n", [("lattice", 10), ("lattice", 30), ("lattice", 70), ("non_metric", 9), ("non_metric", 40)])
def test_ties_and_non_metric(kind, n):
    rng = np.random.default_rng(77 + n)
    Ds = np.stack([(lattice if kind == "lattice" else non_metric)(rng, n) for _ in range(4)])
    r, ub = device_bound(Ds)
    assert_same(r, Ds, ub, what=f"{kind} n={n}")
    if n <= 10:
        for D, b in zip(Ds, r.bound.cpu().numpy()):
            assert b <= hk.optimum(D)[0] * (1 + 1e-9)


# ---- 5. pi and iters ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [8, 50, 129])
def test_pi_attains_the_bound(n):
    from gnngls_amd import ops
    Ds = instances(n, 3)
    max_iters = 2000
    r, ub = device_bound(Ds, max_iters=max_iters)
    assert_same(r, Ds, ub, max_iters, what=f"n={n}")
    bound, pi, kind = r.bound.cpu().numpy(), r.pi.cpu().numpy(), r.exit_kind.cpu().numpy()
    assert bool((r.iters >= 1).all()) and bool((r.iters <= max_iters).all())
    for b in range(len(Ds)):
        w, deg = one_tree_value(Ds[b], pi[b])
        assert bits(w) == bits(bound[b]), (n, b, w, bound[b])
        if kind[b] == ops.BOUND_EXIT_TOUR:
            assert (deg == 2).all()
            if n <= 12:
                assert abs(bound[b] - hk.optimum(Ds[b])[0]) <= 1e-9 * bound[b]
    r2, _ = device_bound(Ds, max_iters=max_iters, want_pi=False)
    assert r2.pi is None and torch.equal(r2.bound, r.bound) and torch.equal(r2.iters, r.iters)


# ---- 6. batching -------------------------------------------------------------------------------------------------------------
def test_batch_rows_equal_single_calls():
    Ds = instances(20, 300)
    D = dev(Ds)
    nn = nn_length(D).cpu().numpy()
    ub = nn * (1.0 + 0.001 * np.arange(300))           # distinct upper bounds
    r, _ = device_bound(Ds, ub=ub)
    rows = [0, 1, 63, 64, 150, 255, 256, 299]
    want = oracle_bounds(Ds[rows], ub[rows])
    assert np.array_equal(bits(r.bound.cpu().numpy()[rows]), bits(want))
    for k in rows:
        one, _ = device_bound(Ds[k:k + 1], ub=ub[k:k + 1])
        assert torch.equal(one.bound, r.bound[k:k + 1]) and torch.equal(one.pi, r.pi[k:k + 1])
        assert torch.equal(one.iters, r.iters[k:k + 1]) and torch.equal(one.exit_kind, r.exit_kind[k:k + 1])


def test_more_workgroups_than_fit_at_once_and_empty_batch():
    from gnngls_amd import ops
    Ds = instances(8, 3000)
    r, ub = device_bound(Ds)
    first, _ = device_bound(Ds[:10], ub=ub[:10])
    for name in ("bound", "pi", "iters", "exit_kind", "status"):
        assert torch.equal(getattr(r, name)[:10], getattr(first, name)), name
    assert np.array_equal(bits(r.bound.cpu().numpy()[-4:]), bits(oracle_bounds(Ds[-4:], ub[-4:])))
    e = ops.one_tree_bound(torch.zeros((0, 8, 8), dtype=torch.float64, device="cuda"), torch.zeros((0,), dtype=torch.float64, device="cuda"))
    assert e.bound.shape == (0,) and e.pi.shape == (0, 8) and e.iters.shape == (0,) and e.exit_kind.shape == (0,)


# ---- 7. validity at benchmark size -------------------------------------------------------------------------------------------
def test_bound_is_below_proven_optima_tsp50():
    from gnngls_amd.synthetic import random_instances
    z = np.load(os.path.join(ROOT, "bench_data", "exact_optima_tsp50_seed2024.npz"))
    proven = np.flatnonzero(z["proven"])[:8]
    Dall, _ = random_instances(np.random.default_rng(2024), 1024, 50)
    Ds = Dall[proven]
    r, ub = device_bound(Ds)
    assert_same(r, Ds, ub, what="tsp50 proven")
    opt = z["optimum"][proven] if "optimum" in z.files else z["opt"][proven]
    assert (r.bound.cpu().numpy() <= opt * (1 + 1e-9)).all()


# ---- 8. status ---------------------------------------------------------------------------------------------------------------
def test_asymmetric_matrix_is_flagged():
    from gnngls_amd import _lib, ops
    Ds = instances(20, 4).copy()
    Ds[2, 7, 11] = np.nextafter(Ds[2, 7, 11], np.inf)  # one ulp in one triangle
    D = dev(Ds)
    ub = nn_length(D)
    bound = torch.full((4,), -7.0, dtype=torch.float64, device="cuda")
    pi = torch.full((4, 20), -7.0, dtype=torch.float64, device="cuda")
    iters = torch.full((4,), -7, dtype=torch.int32, device="cuda")
    kind, status = iters.clone(), iters.clone()
    L = _lib.load()
    assert L.gnngls_one_tree_bound(_lib.ptr(D), _lib.ptr(ub), 4, 20, 2000, _lib.ptr(bound), _lib.ptr(pi), _lib.ptr(iters),
                                   _lib.ptr(kind), _lib.ptr(status), _lib.current_stream()) == 0
    torch.cuda.synchronize()
    assert status.tolist() == [0, 0, ops.STATUS_ASYMMETRIC, 0]
    assert bool(torch.isnan(bound[2])) and int(iters[2]) == -7 and int(kind[2]) == -7 and bool((pi[2] == -7.0).all())
    ok = [0, 1, 3]
    assert np.array_equal(bits(bound.cpu().numpy()[ok]), bits(oracle_bounds(Ds[ok], ub.cpu().numpy()[ok])))
    with pytest.raises(ValueError, match="symmetric"):
        ops.one_tree_bound(D, ub)


# ---- 9. surface --------------------------------------------------------------------------------------------------------------
def test_torch_op_and_profile_kind():
    import gnngls_amd.torch_ops  # noqa: F401
    from gnngls_amd import _lib, ops
    D = dev(instances(12, 4))
    ub = nn_length(D)
    _lib.profile_enable(True)
    try:
        r = ops.one_tree_bound(D, ub, max_iters=500)
        prof = _lib.profile_collect()
    finally:
        _lib.profile_enable(False)
    assert prof["one_tree_bound"][1] == 1 and prof["one_tree_bound"][0] > 0.0 and prof["insertion"][1] == 0
    out = torch.ops.gnngls.one_tree_bound(D, ub, 500)
    for a, b in zip(out, (r.bound, r.pi, r.iters, r.exit_kind, r.status)):
        assert torch.equal(a, b)


def test_solve_batch_lower_bound():
    from gnngls_amd import pipeline
    Ds = instances(20, 4)
    D = dev(Ds)
    kw = dict(guides=("weight",), max_outer_iters=3)
    a = pipeline.solve_batch(D, **kw)
    b = pipeline.solve_batch(D, lower_bound=True, **kw)
    assert a.lower_bound is None and a.bound_exit is None and "bound_s" not in a.timing
    assert torch.equal(a.best_tour, b.best_tour) and torch.equal(a.best_cost, b.best_cost)
    want = oracle_bounds(Ds, b.best_cost.cpu().numpy())
    assert np.array_equal(bits(b.lower_bound.cpu().numpy()), bits(want))
    assert b.bound_exit.shape == (4,) and b.timing["bound_s"] > 0.0
    assert bool((b.lower_bound <= b.best_cost * (1 + 1e-9)).all())


def test_single_graph_mirror():
    import gnngls_amd
    from gnngls_amd import datasets
    from gnngls_amd.algorithms import _attr_matrix
    from test_n3_ingestion_cpu import names
    fix = os.path.join(ROOT, "tests", "golden", "n3_tsp12")
    G = datasets.read_gpickle(os.path.join(fix, names()[0]))
    D = _attr_matrix(G, "weight")
    tour = list(range(len(G.nodes))) + [0]
    lb = gnngls_amd.lower_bound(G, tour)
    assert type(lb) is float and bits(lb) == bits(ot.lower_bound(D, gnngls_amd.tour_cost(G, tour)))
    assert lb <= gnngls_amd.optimal_cost(G) * (1 + 1e-9)
    nn = dev(D[None])
    assert bits(gnngls_amd.lower_bound(G)) == bits(ot.lower_bound(D, float(nn_length(nn)[0])))


def test_cli_lower_bound_columns(tmp_path):
    fix = os.path.join(ROOT, "tests", "golden", "n3_tsp12")
    data = tmp_path / "tsp12"
    shutil.copytree(fix, data)
    mdir = tmp_path / "models" / "tsp12"
    mdir.mkdir(parents=True)
    json.dump({"embed_dim": 128, "n_layers": 3, "n_heads": 8}, open(mdir / "params.json", "w"))
    seven = ["instance", "time", "opt_cost", "cost", "best_cost", "gap", "dt"]
    for extra in (["--lower_bound"], []):
        run_dir = tmp_path / ("runs" + "".join(extra).replace("-", ""))
        subprocess.check_call([sys.executable, os.path.join(ROOT, "scripts", "test.py"), str(data / "test.txt"),
                               str(mdir / "checkpoint_best_val.pt"), str(run_dir), "weight", "--time_limit", "0.3", "--use_gpu"] + extra,
                              cwd=ROOT)
        df = pickle.load(open(next(run_dir.glob("*.pkl")), "rb"))
        if not extra:
            assert list(df.columns) == seven
            continue
        assert sorted(df.columns) == sorted(seven + ["lower_bound", "gap_bound"])
        assert (df["lower_bound"] <= df["opt_cost"] * (1 + 1e-9)).all()
        g = df.groupby("instance")
        assert (g["lower_bound"].nunique() == 1).all()
        last = g.last()
        assert np.allclose(last["gap_bound"], (last["best_cost"] / last["lower_bound"] - 1) * 100, rtol=0, atol=1e-12)
        assert (last["gap_bound"] >= -1e-7).all()
