"""GPU checks of beam-search decoding (ops.beam_search: beam_search_kernel in beam_kernels.hip) against its NumPy definition,
host.beam_search.

Everything is compared as bit patterns: the best tour, its score and cost, the number of beams, the status, every beam row and
the -1 / NaN padding.  Sizes sit where there are fewer candidates than `width` (n = 3, 4, 5), at the lane and bitmask-word edges
(63 / 64 / 65, 129), at the widest beam and at the largest n; one case keeps its visited bits in LDS and one in the global
workspace.  Scores: Euclidean, non-metric, integer-valued with heavy ties, constant, mixed signed zeros, negative, and a batch
with a refused instance between two good ones.
"""
import os
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


def dev(x, dtype=torch.float64):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dtype).cuda()


KINDS = {
    "euclid": lambda rng, n: euclid(rng, n),
    "nonmetric": lambda rng, n: rng.random((n, n)) * 10.0,
    "integer": lambda rng, n: rng.integers(0, 4, (n, n)).astype(np.float64),
    "constant": lambda rng, n: np.full((n, n), 0.75),
    "zeros": lambda rng, n: np.where(rng.random((n, n)) < 0.5, -0.0, 0.0),
    "negative": lambda rng, n: np.round(rng.random((n, n)) * 8.0 - 6.0, 1),
}


def nan_instance(rng, n):
    S = rng.random((n, n))
    S[n - 1, 1] = np.nan
    return S


def check_against_host(S, D, width, depot, select, use_d=True):
    """Runs the batch on the device and every instance on the host; everything is compared as bits."""
    B, n, _ = S.shape
    r = ops.beam_search_launch(dev(S), width, depot, dev(D) if use_d else None, select, want_beams=True)
    torch.cuda.synchronize()
    lean = ops.beam_search_launch(dev(S), width, depot, dev(D) if use_d else None, select, want_beams=False)
    assert lean.beam_tours is None and lean.beam_score is None and lean.beam_cost is None
    for b in range(B):
        o = host.beam_search(S[b], width, depot=depot, D=D[b] if use_d else None, select=select)
        what = f"instance {b} (n={n}, width={width}, depot={depot}, select={select}, D={use_d})"
        assert int(r.status[b]) == o.status and int(r.n_beams[b]) == o.n_beams, what
        assert np.array_equal(r.beam_tours[b].cpu().numpy(), o.beam_tours), what
        assert np.array_equal(bits(r.beam_score[b].cpu().numpy()), bits(o.beam_score)), what
        assert np.array_equal(bits(r.beam_cost[b].cpu().numpy()), bits(o.beam_cost)), what
        for x in (r, lean):
            assert np.array_equal(x.best_tour[b].cpu().numpy(), o.best_tour), what
            assert bits(x.best_score[b].item()) == bits(o.best_score) and bits(x.best_cost[b].item()) == bits(o.best_cost), what
            assert int(x.status[b]) == o.status and int(x.n_beams[b]) == o.n_beams, what
    ok = (r.status == 0).cpu().numpy()
    if use_d and ok.any():
        again = ops.tour_cost(r.best_tour[torch.from_numpy(ok).cuda()].contiguous(), dev(D[ok]))
        assert np.array_equal(bits(again.cpu().numpy()), bits(r.best_cost.cpu().numpy()[ok]))
    return r


CONFIGS = [(0, "cost", True), (-1, "score", False), (-1, "score", True)]          # (depot: -1 = n - 1, select, with D)


def run_batches(n, width, batches, configs=CONFIGS):
    rng = np.random.default_rng(1000 * n + width)
    for kinds in batches:
        S = np.stack([nan_instance(rng, n) if k == "nan" else KINDS[k](rng, n) for k in kinds])
        S[0][np.diag_indices(n)] = np.nan                                          # the diagonal is never read
        D = np.stack([euclid(rng, n) for _ in kinds])
        for depot, select, use_d in configs:
            r = check_against_host(S, D, width, depot % n, select, use_d)
            for b, k in enumerate(kinds):
                assert int(r.status[b]) == (ops.BEAM_BAD_SCORE if k == "nan" else 0)


ALL_BATCHES = [("euclid", "nonmetric", "integer"), ("constant", "zeros", "negative"), ("euclid", "nan", "integer")]


# fewer candidates than width: n_beams < width wherever width > (n-1)!
@pytest.mark.parametrize("width", [1, 2, 3, 7, 64])
@pytest.mark.parametrize("n", [3, 4, 5])
def test_small_trees(n, width):
    run_batches(n, width, ALL_BATCHES)
    S = KINDS["nonmetric"](np.random.default_rng(n), n)[None]
    r = ops.beam_search(dev(S), width, want_beams=True)
    leaves = [2, 6, 24][n - 3]
    assert int(r.n_beams[0]) == min(width, leaves)
    assert (r.beam_tours[0, min(width, leaves):] == -1).all()


# the lane and bitmask-word edges
@pytest.mark.parametrize("width", [1, 2, 63, 64, 65, 256])
@pytest.mark.parametrize("n", [63, 64, 65, 100, 129])
def test_lane_and_word_edges(n, width):
    run_batches(n, width, ALL_BATCHES)


# the widest beam; at n = 20 the first steps have fewer candidates than beams
@pytest.mark.parametrize("n", [20, 65])
def test_widest_beam(n):
    run_batches(n, 1024, [("euclid", "integer", "constant"), ("negative", "nan", "zeros")], configs=CONFIGS[:2])


def _workspace_without_masks(n, width):
    r16 = lambda x: (x + 15) & ~15  # noqa: E731
    return r16((n - 1) * width * 4) + r16(width * (n + 1) * 4)


# The visited bits, 2 * width * ceil(n / 64) words, stay in LDS while they fit beside 45,072 B of other state (width 1,024) under the
# 80 KiB a workgroup may take: 77,840 B at n = 65 .. 128, 94,224 B at n = 129, which therefore keeps them in the global workspace.
def test_visited_bits_in_lds_and_in_the_workspace():
    assert ops.beam_search_workspace_bytes(1, 128, 1024) == _workspace_without_masks(128, 1024)
    assert ops.beam_search_workspace_bytes(1, 129, 1024) == _workspace_without_masks(129, 1024) + 2 * 1024 * 3 * 8
    run_batches(128, 1024, [("euclid", "integer")], configs=CONFIGS[:1])          # LDS
    run_batches(129, 1024, [("euclid", "integer")], configs=CONFIGS[:2])          # global workspace


# the largest n: 16 bitmask words per beam, in LDS at both widths
@pytest.mark.parametrize("width", [8, 64])
def test_largest_instance(width):
    assert ops.beam_search_workspace_bytes(1, 1024, width) == _workspace_without_masks(1024, width)
    run_batches(1024, width, [("euclid", "integer")], configs=CONFIGS[:2])


@pytest.mark.parametrize("n", [5, 64, 100])
def test_width_one_is_nearest_neighbor(n):
    rng = np.random.default_rng(n)
    S = dev(np.stack([KINDS["integer"](rng, n) for _ in range(3)]))
    for depot in (0, n - 1, n // 2):
        r = ops.beam_search(S, 1, depot)
        assert torch.equal(r.best_tour, ops.nearest_neighbor(S, depot)) and (r.n_beams == 1).all()


def test_refused_instance_raises_and_spares_its_neighbours():
    rng = np.random.default_rng(3)
    S = np.stack([euclid(rng, 30), nan_instance(rng, 30), euclid(rng, 30)])
    S[1, 3, 4] = np.inf
    with pytest.raises(ValueError, match=r"instances \[1\]"):
        ops.beam_search(dev(S), 16)
    r = ops.beam_search_launch(dev(S), 16, D=dev(S), select="cost", want_beams=True)
    assert r.status.tolist() == [0, 1, 0] and r.n_beams.tolist() == [16, 0, 16]
    assert (r.best_tour[1] == -1).all() and (r.beam_tours[1] == -1).all() and torch.isnan(r.beam_score[1]).all()
    alone = ops.beam_search(dev(S[2:]), 16, D=dev(S[2:]), select="cost", want_beams=True)
    assert torch.equal(alone.beam_tours[0], r.beam_tours[2]) and torch.equal(alone.beam_score[0], r.beam_score[2])


def test_range_errors_raise_without_a_launch():
    S = dev(np.ones((2, 6, 6)))
    for kw in (dict(width=0), dict(width=1025), dict(width=4, depot=6), dict(width=4, depot=-1), dict(width=4, select="cost")):
        with pytest.raises(_lib.GnnglsHipError, match="beam_search"):
            ops.beam_search(S, **kw)
    with pytest.raises(ValueError):
        ops.beam_search(S, 4, select="shortest")
    with pytest.raises(_lib.GnnglsHipError, match="n=2"):
        ops.beam_search(dev(np.ones((1, 2, 2))), 1)
    with pytest.raises(_lib.GnnglsHipError, match="n=1025"):
        ops.beam_search(torch.ones((1, 1025, 1025), dtype=torch.float64, device="cuda"), 1)
    need = ops.beam_search_workspace_bytes(2, 6, 4)
    with pytest.raises(_lib.GnnglsHipError, match="too small"):
        ops.beam_search(S, 4, workspace=torch.empty(need - 1, dtype=torch.uint8, device="cuda"))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    a, b = ops.beam_search(S, 4, workspace=ws), ops.beam_search(S, 4)
    assert torch.equal(a.best_tour, b.best_tour) and a.best_tour[0].tolist() == [0, 1, 2, 3, 4, 5, 0]
    torch.cuda.synchronize()


def test_torch_op_and_graph_mirror():
    import networkx as nx

    import gnngls_amd.torch_ops  # noqa: F401
    from gnngls_amd import algorithms
    rng = np.random.default_rng(8)
    n = 12
    D, R = euclid(rng, n), rng.random((n, n))
    R = (R + R.T) / 2
    out = torch.ops.gnngls.beam_search(dev(R[None]), dev(D[None]), 8, 2, "cost")
    o = host.beam_search(R, 8, depot=2, D=D, select="cost")
    assert out[0][0].cpu().tolist() == o.best_tour.tolist() and np.array_equal(out[5][0].cpu().numpy(), o.beam_tours)
    assert np.array_equal(bits(out[6][0].cpu().numpy()), bits(o.beam_score)) and out[4].tolist() == [0]
    G = nx.complete_graph(n)
    nx.set_edge_attributes(G, {(u, v): float(D[u, v]) for u, v in G.edges}, "weight")
    nx.set_edge_attributes(G, {(u, v): float(R[u, v]) for u, v in G.edges}, "regret_pred")
    assert algorithms.beam_search(G, 2, 8) == o.best_tour.tolist()
    assert algorithms.beam_search(G, 2, 8, select="score") == host.beam_search(R, 8, depot=2).best_tour.tolist()
    assert algorithms.beam_search(G, 0, 1, guide="weight") == host.beam_search(D, 1).best_tour.tolist()
