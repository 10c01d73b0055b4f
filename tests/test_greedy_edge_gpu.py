"""GPU checks of greedy edge matching (ops.greedy_edge: greedy_edge_kernel in greedy_edge_kernels.hip) against its NumPy definition,
host.greedy_edge.

Everything is compared as bit patterns: the tour, its score and cost, the edges in acceptance order, the rounds and the status.
Sizes sit where there is no choice (n = 3), one choice (4), the first rejected subtour edge (5), at the lane and wavefront edges of
the row scan (63 / 64 / 65, 100, 129: the first sizes with more rows than wavefronts) and at the largest n.  Scores: Euclidean,
non-metric, integer-valued with heavy ties, constant, mixed signed zeros, negative -- all made bitwise symmetric, as the kernel
reads row u for node u -- mixed inside one batch, and a batch with a refused instance between two good ones.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gnngls_amd import _lib, host, ops  # noqa: E402


def bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.uint64)


def euclid(rng, n):
    pos = rng.random((n, 2))
    return np.linalg.norm(pos[:, None] - pos[None], axis=2)


def mirrored(M):
    """The upper triangle on both sides, bit for bit (signed zeros included); the diagonal stays."""
    U = np.triu(M, 1)
    return np.where(np.tri(M.shape[0], k=-1, dtype=bool), U.T, np.where(np.eye(M.shape[0], dtype=bool), M, U))


def dev(x, dtype=torch.float64):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dtype).cuda()


KINDS = {
    "euclid": lambda rng, n: euclid(rng, n),
    "nonmetric": lambda rng, n: mirrored(rng.random((n, n)) * 10.0),
    "integer": lambda rng, n: mirrored(rng.integers(0, 4, (n, n)).astype(np.float64)),
    "constant": lambda rng, n: np.full((n, n), 0.75),
    "zeros": lambda rng, n: mirrored(np.where(rng.random((n, n)) < 0.5, -0.0, 0.0)),
    "negative": lambda rng, n: mirrored(np.round(rng.random((n, n)) * 8.0 - 6.0, 1)),
}


def nan_instance(rng, n):
    S = mirrored(rng.random((n, n)))
    S[n - 1, 1] = S[1, n - 1] = np.nan
    return S


def chain(n):
    p = 2.0 ** np.arange(n)
    return np.abs(p[:, None] - p[None])


_HOST = {}


def host_result(S, depot, D):
    """host.greedy_edge, computed once per (matrix, depot, D) of this module."""
    key = (S.tobytes(), depot, None if D is None else D.tobytes())
    if key not in _HOST:
        _HOST[key] = host.greedy_edge(S, depot=depot, D=D)
    return _HOST[key]


def check_against_host(S, D, depot, use_d=True):
    """Runs the batch on the device, with and without the edges, and every instance on the host; everything is compared as bits."""
    B, n, _ = S.shape
    for b in range(B):
        assert np.array_equal(bits(S[b])[~np.eye(n, dtype=bool)], bits(S[b].T)[~np.eye(n, dtype=bool)]), "the test's own S is symmetric"
    r = ops.greedy_edge_launch(dev(S), depot, dev(D) if use_d else None, want_edges=True)
    lean = ops.greedy_edge_launch(dev(S), depot, dev(D) if use_d else None, want_edges=False)
    torch.cuda.synchronize()
    assert lean.edges is None
    for b in range(B):
        o = host_result(S[b], depot, D[b] if use_d else None)
        what = f"instance {b} (n={n}, depot={depot}, D={use_d})"
        assert np.array_equal(r.edges[b].cpu().numpy(), o.edges), what              # first: this localises a mismatch
        for x in (r, lean):
            assert int(x.status[b]) == o.status and int(x.rounds[b]) == o.rounds, what
            assert np.array_equal(x.tour[b].cpu().numpy(), o.tour), what
            assert bits(x.score[b].item()) == bits(o.score) and bits(x.cost[b].item()) == bits(o.cost), what
    ok = (r.status == 0).cpu().numpy()
    if use_d and ok.any():
        again = ops.tour_cost(r.tour[torch.from_numpy(ok).cuda()].contiguous(), dev(D[ok]))
        assert np.array_equal(bits(again.cpu().numpy()), bits(r.cost.cpu().numpy()[ok]))
    return r


CONFIGS = [(0, True), (-1, False), (-1, True), (0, False)]                        # (depot: -1 = n - 1, with D)
ALL_BATCHES = [("euclid", "nonmetric", "integer"), ("constant", "zeros", "negative"), ("euclid", "nan", "integer")]


def run_batches(n, batches, configs=CONFIGS):
    rng = np.random.default_rng(1000 * n + 7)
    for kinds in batches:
        S = np.stack([nan_instance(rng, n) if k == "nan" else KINDS[k](rng, n) for k in kinds])
        S[0][np.diag_indices(n)] = np.nan                                          # the diagonal is never used
        D = np.stack([euclid(rng, n) for _ in kinds])
        for depot, use_d in configs:
            r = check_against_host(S, D, depot % n, use_d)
            for b, k in enumerate(kinds):
                assert int(r.status[b]) == (ops.GREEDY_EDGE_BAD_SCORE if k == "nan" else 0)


# no choice, one choice, the first rejected subtour edge
@pytest.mark.parametrize("n", [3, 4, 5])
def test_smallest_instances(n):
    run_batches(n, ALL_BATCHES)
    for depot in range(n):
        check_against_host(np.stack([KINDS["integer"](np.random.default_rng(n), n), KINDS["constant"](None, n)]),
                           np.ones((2, n, n)), depot)


# the lane and wavefront edges of the row scan; from n = 65 on more rows than the workgroup has wavefronts
@pytest.mark.parametrize("n", [63, 64, 65, 100, 129])
def test_lane_and_wavefront_edges(n):
    run_batches(n, ALL_BATCHES)


# the size limit: 16 wavefronts, one thread per node, the largest per-node LDS state
def test_largest_instance():
    n = 1024
    rng = np.random.default_rng(1024)
    S = np.stack([euclid(rng, n), KINDS["integer"](rng, n)])
    D = np.stack([S[0], S[0]])
    r = check_against_host(S, D, n - 1)
    assert int(r.rounds[0]) < 100 < int(r.rounds[1])                               # ties serialise: hundreds of rounds


def test_worst_case_chain_takes_every_round():
    n = 70
    S = np.stack([chain(n), KINDS["euclid"](np.random.default_rng(70), n)])
    r = check_against_host(S, S, 0)
    assert int(r.rounds[0]) == n - 1 and r.tour[0].tolist() == list(range(n)) + [0]
    assert r.edges[0].tolist() == [[i, i + 1] for i in range(n - 1)] + [[0, n - 1]]


# every key ties: the (i, j) part of the arg-min decides everything
def test_constant_and_zero_scores():
    n = 65
    rng = np.random.default_rng(65)
    S = np.stack([KINDS["constant"](rng, n), KINDS["zeros"](rng, n), np.zeros((n, n)), np.full((n, n), -2.5)])
    D = np.stack([euclid(rng, n) for _ in range(4)])
    for depot in (0, 33, n - 1):
        r = check_against_host(S, D, depot)
        want = [[0, 1]] + [[k, k + 2] for k in range(n - 2)] + [[n - 2, n - 1]]
        for b in range(4):
            assert r.edges[b].tolist() == want
        assert np.array_equal(bits(r.score.cpu().numpy()), bits([0.75 * n, 0.0, 0.0, -2.5 * n]))


def test_refused_instance_raises_and_spares_its_neighbours():
    rng = np.random.default_rng(3)
    S = np.stack([euclid(rng, 30), nan_instance(rng, 30), euclid(rng, 30)])
    S[1, 3, 4] = S[1, 4, 3] = np.inf
    with pytest.raises(ValueError, match=r"instances \[1\]"):
        ops.greedy_edge(dev(S))
    r = check_against_host(S, S, 0)
    assert r.status.tolist() == [0, 1, 0] and r.rounds[1].item() == 0
    assert (r.tour[1] == -1).all() and (r.edges[1] == -1).all() and torch.isnan(r.score[1]) and torch.isnan(r.cost[1])
    alone = ops.greedy_edge(dev(S[2:]), D=dev(S[2:]), want_edges=True)
    assert torch.equal(alone.edges[0], r.edges[2]) and torch.equal(alone.tour[0], r.tour[2]) and torch.equal(alone.score[0], r.score[2])


def test_asymmetric_score_raises_before_a_launch():
    S = dev(KINDS["euclid"](np.random.default_rng(4), 12)[None]).repeat(2, 1, 1)
    S[1, 2, 5] += 1.0
    with pytest.raises(ValueError, match=r"instances \[1\] are not bitwise symmetric"):
        ops.greedy_edge(S)


def test_range_errors_raise_without_a_launch():
    S = dev(np.ones((2, 6, 6)))
    for kw in (dict(depot=6), dict(depot=-1)):
        with pytest.raises(_lib.GnnglsHipError, match="greedy_edge: depot"):
            ops.greedy_edge(S, **kw)
    with pytest.raises(_lib.GnnglsHipError, match="n=2"):
        ops.greedy_edge(dev(np.ones((1, 2, 2))))
    with pytest.raises(_lib.GnnglsHipError, match="n=1025"):
        ops.greedy_edge(torch.ones((1, 1025, 1025), dtype=torch.float64, device="cuda"))
    assert ops.greedy_edge(S).tour[0].tolist() == [0, 1, 3, 5, 4, 2, 0]
    torch.cuda.synchronize()


def test_torch_op_and_graph_mirror():
    import networkx as nx

    import gnngls_amd.torch_ops  # noqa: F401
    from gnngls_amd import algorithms
    rng = np.random.default_rng(8)
    n = 12
    D, R = euclid(rng, n), rng.random((n, n))
    R = (R + R.T) / 2
    out = torch.ops.gnngls.greedy_edge(dev(R[None]), dev(D[None]), 2)
    r = ops.greedy_edge_launch(dev(R[None]), 2, dev(D[None]), want_edges=True)
    for x, y in zip(out, (r.tour, r.score, r.cost, r.edges, r.rounds, r.status)):
        assert x.dtype == y.dtype and torch.equal(x.view(torch.int32) if x.dtype == torch.float64 else x,
                                                  y.view(torch.int32) if y.dtype == torch.float64 else y)
    o = host.greedy_edge(R, depot=2, D=D)
    assert out[0][0].tolist() == o.tour.tolist() and out[3][0].tolist() == o.edges.tolist() and out[5].tolist() == [0]
    G = nx.complete_graph(n)
    nx.set_edge_attributes(G, {(u, v): float(D[u, v]) for u, v in G.edges}, "weight")
    nx.set_edge_attributes(G, {(u, v): float(R[u, v]) for u, v in G.edges}, "regret_pred")
    assert algorithms.greedy_edge(G, 2) == o.tour.tolist()
    assert algorithms.greedy_edge(G) == host.greedy_edge(R).tour.tolist()
    assert algorithms.greedy_edge(G, 5, guide="weight") == host.greedy_edge(D, depot=5).tour.tolist()


def test_bench_script_on_a_small_load(tmp_path):
    out = tmp_path / "greedy_edge.json"
    subprocess.check_call([sys.executable, os.path.join(ROOT, "scripts", "bench_greedy_edge.py"), "--shapes", "100x16", "--out", str(out)],
                          cwd=ROOT)
    res = json.load(open(out))
    (s,) = res["shapes"]
    assert s["n"] == 100 and s["instances"] == 16
    t = s["device_time"]
    assert t["greedy_edge"]["device_ms_median"] > 0 and t["argsort_keys_device"]["device_ms_median"] > 0 and t["host_acceptance_ms"] > 0
    assert t["same_tours_as_argsort"] is True and 1 <= s["rounds"]["mean"] <= s["rounds"]["max"] <= 99
    assert set(s["guide_scores"]) == set(s["decode"]) == {"weight", "alpha", "regret_synthetic"}
    for cell in s["decode"].values():
        assert cell["mean_gap_pct"] >= cell["mean_gap_pct_after_or_opt"] > 0 and cell["device_ms_once"] > 0
    assert s["nearest_neighbor_gap_pct"] > 0 and s["beam_128_weight_gap_pct"] > 0 and s["guided_equal_time"]["mean_gap_pct"] >= 0
