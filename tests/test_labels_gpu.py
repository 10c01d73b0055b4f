"""Regret labels on the MI355X (gnngls_regret_labels, gnngls_amd.labels): per-job bit-exact parity with the oracle on a
host-built D', exact labels against Held-Karp, the repair rounds, determinism and chunk independence, and the whole
generate -> preprocess -> train -> test workflow."""
import itertools
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_labels_cpu import held_karp_raw, n3_instances

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tour_edges(t):
    return {frozenset((int(t[p]), int(t[p + 1]))) for p in range(len(t) - 1)}


def _sample_jobs(base, n, rng, k):
    """Edges off the base tour: depot edges (0, j), edges whose endpoints sit two positions apart, and random ones."""
    on = _tour_edges(base)
    off = [(i, j) for i, j in itertools.combinations(range(n), 2) if frozenset((i, j)) not in on]
    depot = [e for e in off if e[0] == 0]
    two = [tuple(sorted((base[p], base[p + 2]))) for p in range(n - 1)]
    two = [e for e in two if frozenset(e) not in on]
    pick = [depot[0], depot[-1], two[0], two[len(two) // 2]]
    pick += [off[q] for q in rng.choice(len(off), k, replace=False)]
    return sorted(set(pick))


@pytest.mark.parametrize("n", [20, 100, 131])
def test_fixed_edge_jobs_match_the_oracle_bit_for_bit(n):
    from gnngls_amd import labels, ops
    from gnngls_amd.synthetic import random_instances
    from oracle import gls_oracle as go
    B = 2
    D, _ = random_instances(np.random.default_rng(100 + n), B, n)
    rng = np.random.default_rng(n)
    Dd = torch.from_numpy(D).cuda()
    base = ops.nearest_neighbor(Dd)
    bh = base.cpu().numpy()
    N = n * (n - 1) // 2
    mask = torch.zeros((B, N), dtype=torch.bool)
    jobs = []
    for b in range(B):
        for i, j in _sample_jobs(bh[b].tolist(), n, rng, 3 if n > 100 else 5):
            mask[b, labels.edge_rank(i, j, n)] = True
            jobs.append((b, i, j))
    ec = torch.full((B, N), float("inf"), dtype=torch.float64, device="cuda")
    ec, _, _, _, st = labels.fixed_edge_labels(Dd, base, mask.cuda(), ec)
    assert (st.cpu() == 0).all()
    ech = ec.cpu().numpy()
    K = labels.LABEL_ITERS
    for b, i, j in jobs:
        Dp = labels.fixed_edge_matrix(D[b], i, j)
        o = go.guided_local_search(Dp, Dp[None], bh[b], go.tour_cost(bh[b], Dp), perturbation_moves=labels.PERTURBATION_MOVES,
                                   max_outer_iters=K, want_penalty=False, trace_cap=1)
        label = go.tour_cost(o["best_tour"], D[b])
        assert frozenset((i, j)) in _tour_edges(o["best_tour"])
        assert np.float64(ech[b, labels.edge_rank(i, j, n)]).tobytes() == np.float64(label).tobytes(), (n, b, i, j)
        # the same job through the search entry directly: best tour and its D'-cost bits
        Dpd = torch.from_numpy(Dp[None]).cuda()
        t0 = base[b:b + 1].contiguous()
        r = ops.gls_run(Dpd, Dpd[None].contiguous(), t0, ops.tour_cost(t0, Dpd), perturbation_moves=labels.PERTURBATION_MOVES,
                        max_outer_iters=K)
        assert r.best_tour[0].tolist() == o["best_tour"]
        assert np.float64(r.best_cost[0].item()).tobytes() == np.float64(o["best_cost"]).tobytes()


def test_exact_labels_on_the_n3_fixtures():
    from gnngls_amd import labels
    insts = n3_instances()
    D = np.stack([d for d, _ in insts])
    res = labels.regret_labels(D, base_tour=[t for _, t in insts])
    assert (res.status.cpu() == labels.STATUS_OK).all() and (res.rounds.cpu() == 1).all()
    n = D.shape[1]
    ec, rg, on = res.edge_cost.cpu().numpy(), res.regret.cpu().numpy(), res.in_solution.cpu().numpy()
    for b, (Db, base) in enumerate(insts):
        assert res.tour[b].tolist() == base
        opt = ec[b][on[b]][0]
        for r, (i, j) in enumerate(itertools.combinations(range(n), 2)):
            if on[b, r]:
                assert rg[b, r] == 0.0 and ec[b, r] == opt
                continue
            t = held_karp_raw(labels.fixed_edge_matrix(Db, i, j))
            exact = sum(Db[t[p], t[p + 1]] for p in range(n))
            assert abs(ec[b, r] - exact) <= 1e-12 * exact, (b, i, j)
            assert rg[b, r] == (ec[b, r] - opt) / opt and rg[b, r] >= 0.0


def _check_invariants(D, res):
    from gnngls_amd.labels import edge_rank
    B, n, _ = D.shape
    tour, ec, rg, on = res.tour.cpu().numpy(), res.edge_cost.cpu().numpy(), res.regret.cpu().numpy(), res.in_solution.cpu().numpy()
    for b in range(B):
        t = tour[b].tolist()
        assert t[0] == t[-1] == 0 and sorted(t[:-1]) == list(range(n))
        assert on[b].sum() == n and all(on[b, edge_rank(t[p], t[p + 1], n)] for p in range(n))
        cost = 0.0
        for p in range(n):
            cost += D[b, t[p], t[p + 1]]
        assert res.cost[b].item() == cost == ec[b].min()
        assert (rg[b] >= 0).all() and (rg[b][on[b]] == 0.0).all() and np.isfinite(rg[b]).all()


def test_repair_rounds_from_a_nearest_neighbour_base():
    """Seed chosen with the oracle: fixed-edge searches from the bare nearest-neighbour tours of these TSP20 instances find
    cheaper tours for every instance, so every instance goes through a repair round."""
    from gnngls_amd import labels
    from gnngls_amd.synthetic import random_instances
    D, _ = random_instances(np.random.default_rng(11), 8, 20)
    res = labels.regret_labels(D, solve_iters=0)
    assert (res.rounds.cpu() > 1).all()
    assert not np.isin(res.status.cpu().numpy(), [labels.STATUS_WATCHDOG, labels.STATUS_EDGE_LOST]).any()
    _check_invariants(D, res)


def test_labels_are_deterministic_and_chunk_independent():
    from gnngls_amd import labels
    from gnngls_amd.synthetic import random_instances
    D, _ = random_instances(np.random.default_rng(21), 64, 20)
    a = labels.regret_labels(D)
    b = labels.regret_labels(D)
    for name in ("tour", "cost", "in_solution", "regret", "edge_cost", "rounds", "status"):
        x, y = getattr(a, name).cpu().numpy(), getattr(b, name).cpu().numpy()
        assert x.tobytes() == y.tobytes(), name
    _check_invariants(D, a)
    k = 37
    alone = labels.regret_labels(D[k:k + 1])
    split = labels.regret_labels(D, chunk_jobs=100)       # 170 jobs per instance: every instance spans two or three chunks
    for name in ("tour", "cost", "regret", "edge_cost", "rounds", "status"):
        x = getattr(alone, name).cpu().numpy()[0]
        assert x.tobytes() == getattr(a, name).cpu().numpy()[k].tobytes(), name
        assert x.tobytes() == getattr(split, name).cpu().numpy()[k].tobytes(), name


def _run(args, limit):
    p = subprocess.run([sys.executable] + args, cwd=ROOT, capture_output=True, text=True, timeout=limit)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    return p


def test_generate_preprocess_train_test(tmp_path):
    from gnngls_amd.datasets import read_gpickle
    from gnngls_amd.labels import edge_rank
    data, tb, runs = tmp_path / "tsp12", tmp_path / "tb", tmp_path / "runs"
    s = os.path.join(ROOT, "scripts")
    _run([os.path.join(s, "generate_instances.py"), "40", "12", str(data), "--seed", "1", "--use_gpu"], 600)
    names = sorted(p.name for p in data.glob("*.pkl"))
    assert len(names) == 40 and all(len(x) == 36 for x in names)
    for name in names:
        G = read_gpickle(data / name)
        n = len(G.nodes)
        assert list(G.edges) == list(itertools.combinations(range(n), 2))
        tour = [0]
        on = [e for e in G.edges if G.edges[e]["in_solution"]]
        assert len(on) == n
        adj = {v: [] for v in range(n)}
        for i, j in on:
            adj[i].append(j)
            adj[j].append(i)
        while len(tour) <= n:
            nxt = [v for v in adj[tour[-1]] if len(tour) < 2 or v != tour[-2]][0]
            tour.append(nxt)
        assert tour[-1] == 0 and sorted(tour[:-1]) == list(range(n))
        for e in G.edges:
            d = G.edges[e]
            assert type(d["weight"]) is np.float64 and d["features"].dtype == np.float32 and isinstance(d["regret"], float)
            assert d["regret"] >= 0.0 and (d["regret"] == 0.0 if d["in_solution"] else True)
            assert edge_rank(e[0], e[1], n) == list(G.edges).index(e)
    _run([os.path.join(s, "preprocess_dataset.py"), str(data), "--n_train", "30", "--n_val", "5", "--n_test", "5", "--seed", "1"], 300)
    _run([os.path.join(s, "train.py"), str(data), str(tb), "--n_epochs", "1", "--use_gpu", "--num_workers", "0"], 900)
    ck = next(tb.iterdir()) / "checkpoint_final.pt"
    assert ck.is_file()
    _run([os.path.join(s, "test.py"), str(data / "test.txt"), str(ck), str(runs), "regret_pred", "--time_limit", "0.1", "--use_gpu"], 600)
    df = pickle.load(open(next(runs.glob("*.pkl")), "rb"))
    assert df["instance"].nunique() == 5
