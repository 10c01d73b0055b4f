"""CPU checks of the regret-label path (gnngls_amd.labels, gnngls_regret_labels, scripts/preprocess_dataset.py): the
fixed-edge offset and line-graph ranks, the label budget against exact constrained optima (oracle on D' vs Held-Karp on D'),
the dataset split / scaler script, and the host side of the new C entries."""
import ctypes
import itertools
import math
import os
import pickle
import subprocess
import sys

import networkx as nx
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N3 = os.path.join(ROOT, "tests", "golden", "n3_tsp12")


def held_karp_raw(D):
    """Exact optimum of D (negative entries allowed: held_karp.optimum() treats a negative cost as its error code)."""
    from oracle import held_karp as hk
    D = np.ascontiguousarray(D, dtype=np.float64)
    n = D.shape[0]
    t = np.zeros(n + 1, dtype=np.int32)
    hk.lib().held_karp(D.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), n, t.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
    return t.tolist()


def n3_instances():
    from gnngls_amd.datasets import _tour_from_edges, read_gpickle
    out = []
    for name in sorted(os.listdir(N3)):
        if name.endswith(".pkl") and not name.startswith("scalers"):
            G = read_gpickle(os.path.join(N3, name))
            n = len(G.nodes)
            D = np.zeros((n, n))
            for i, j, d in G.edges(data=True):
                D[i, j] = D[j, i] = d["weight"]
            out.append((D, _tour_from_edges(G)))
    return out


def test_fixed_edge_offset_is_the_power_of_two():
    from gnngls_amd.labels import fixed_edge_matrix, fixed_edge_offset
    rng = np.random.default_rng(5)
    for n in (3, 12, 20, 100, 131, 255):
        D = rng.random((n, n)) * rng.choice([1e-3, 1.0, 7.0, 1e4])
        M = fixed_edge_offset(D)
        x = (2.0 * n) * D.max()
        m, e = math.frexp(M)
        assert m == 0.5 and M >= x and M / 2 < x
    # exact powers of two are kept; the product, not its factors, is rounded once (the device formula)
    D = np.full((4, 4), 0.25)
    assert fixed_edge_offset(D) == 2.0
    D = np.full((3, 3), 1.0 / 3.0)
    assert (2.0 * 3) * (1.0 / 3.0) == 2.0 and fixed_edge_offset(D) == 2.0      # fl(6 * fl(1/3)) = 2 exactly: kept
    assert fixed_edge_offset(np.zeros((3, 3))) == 1.0
    Dp = fixed_edge_matrix(np.full((4, 4), 0.25), 1, 3)
    assert Dp[1, 3] == Dp[3, 1] == 0.25 - 2.0 and Dp[0, 1] == 0.25


def test_line_graph_ranks_round_trip():
    from gnngls_amd.labels import edge_of_rank, edge_rank
    from gnngls_amd.models import LineGraph
    for n in (3, 4, 12, 20, 101):
        pairs = list(itertools.combinations(range(n), 2))
        for r, (i, j) in enumerate(pairs):
            assert edge_rank(i, j, n) == r and edge_rank(j, i, n) == r
            assert edge_of_rank(r, n) == (i, j)
        if n <= 20:
            assert [tuple(e) for e in LineGraph(n).ndata["e"].tolist()] == pairs


def test_default_budget_reproduces_exact_constrained_optima():
    """n3_tsp12 (exact base tours): the oracle's fixed-edge search at the default label budget finds the Held-Karp optimum of
    D' for all 162 non-tour edges -- to 1e-12 relative on the true cost (tour_cost on D)."""
    from gnngls_amd import labels
    from oracle import gls_oracle as go
    insts = n3_instances()
    assert len(insts) == 3
    checked = 0
    for D, base in insts:
        n = D.shape[0]
        on = {frozenset((base[p], base[p + 1])) for p in range(n)}
        for i, j in itertools.combinations(range(n), 2):
            if frozenset((i, j)) in on:
                continue
            Dp = labels.fixed_edge_matrix(D, i, j)
            o = go.guided_local_search(Dp, Dp[None], np.array(base, dtype=np.int32), go.tour_cost(base, Dp),
                                       perturbation_moves=labels.PERTURBATION_MOVES, max_outer_iters=labels.LABEL_ITERS,
                                       want_penalty=False, trace_cap=1)
            t = o["best_tour"]
            assert frozenset((i, j)) in {frozenset((t[p], t[p + 1])) for p in range(n)}
            exact = go.tour_cost(held_karp_raw(Dp), D)
            assert abs(go.tour_cost(t, D) - exact) <= 1e-12 * exact, (i, j)
            checked += 1
    assert checked == 162


def _fake_dataset(path, count, n, seed):
    """Instances in the format of scripts/generate_instances.py with synthetic labels (no GPU needed for the split)."""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import generate_instances as gi
    from gnngls_amd import datasets
    rng = np.random.default_rng(seed)
    os.makedirs(path)
    for _ in range(count):
        G = gi.make_instance(rng, n)
        for e in G.edges:
            G.edges[e]["in_solution"] = False
            G.edges[e]["regret"] = float(rng.random())
        datasets.set_features(G)
        with open(os.path.join(path, rng.bytes(16).hex() + ".pkl"), "wb") as f:
            pickle.dump(G, f, protocol=pickle.HIGHEST_PROTOCOL)


def _preprocess(d, *args):
    return subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "preprocess_dataset.py"), str(d), *args],
                          capture_output=True, text=True, timeout=300)


def test_preprocess_dataset(tmp_path):
    from sklearn.preprocessing import MinMaxScaler

    from gnngls_amd.datasets import TSPDataset, read_gpickle
    d = tmp_path / "data"
    _fake_dataset(str(d), 12, 8, seed=3)
    p = _preprocess(d, "--n_train", "7", "--n_val", "2", "--n_test", "3", "--seed", "1")
    assert p.returncode == 0, p.stderr
    split = {k: (d / f"{k}.txt").read_text().split() for k in ("train", "val", "test")}
    assert [len(split[k]) for k in ("train", "val", "test")] == [7, 2, 3]
    assert sorted(sum(split.values(), [])) == sorted(f for f in os.listdir(d) if f.endswith(".pkl") and f != "scalers.pkl")
    with open(d / "scalers.pkl", "rb") as f:
        scalers = pickle.load(f)
    assert sorted(scalers) == ["features", "regret"]
    for k in scalers:
        ref = MinMaxScaler()
        for name in split["train"]:
            G = read_gpickle(d / name)
            ref.partial_fit(np.vstack([G.edges[e][k] for e in G.edges]))
        assert np.array_equal(ref.data_min_, scalers[k].data_min_) and np.array_equal(ref.data_max_, scalers[k].data_max_)
        assert np.array_equal(ref.scale_, scalers[k].scale_) and np.array_equal(ref.min_, scalers[k].min_)
    # the same seed gives the same split
    d2 = tmp_path / "copy"
    d2.mkdir()
    for name in sum(split.values(), []):
        (d2 / name).write_bytes((d / name).read_bytes())
    assert _preprocess(d2, "--n_train", "7", "--n_val", "2", "--n_test", "3", "--seed", "1").returncode == 0
    assert (d2 / "train.txt").read_text() == (d / "train.txt").read_text()
    # refuses to overwrite
    p = _preprocess(d, "--n_train", "7", "--seed", "1")
    assert p.returncode != 0 and "scalers.pkl already exists" in p.stderr
    ds = TSPDataset(d / "train.txt")
    assert len(ds) == 7
    H = ds[0]
    assert H.ndata["features"].shape == (28, 1) and H.ndata["regret"].shape == (28, 1)


def test_generated_instance_format():
    """Edges in combinations order, weight bit-identical to np.linalg.norm(pos[j] - pos[i]) (generate_instances.py:29-33)."""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import generate_instances as gi
    G = gi.make_instance(np.random.default_rng(0), 9)
    assert list(G.edges) == list(itertools.combinations(range(9), 2))
    for i, j in G.edges:
        w = G.edges[i, j]["weight"]
        assert type(w) is np.float64 and w == np.linalg.norm(G.nodes[j]["pos"] - G.nodes[i]["pos"])
    D = gi.weight_matrix(G)
    assert np.array_equal(D, D.T) and D[2, 5] == G.edges[2, 5]["weight"]


def test_generate_instances_requires_gpu_flag(tmp_path):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "generate_instances.py"), "2", "8", str(tmp_path / "x")],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode != 0 and "--use_gpu" in p.stderr and not (tmp_path / "x").exists()


@pytest.fixture(scope="module")
def lib():
    from gnngls_amd import _lib, build
    build.build()
    return _lib.load()


def test_label_entries_exported_and_checked(lib):
    from gnngls_amd import _lib
    raw = ctypes.CDLL(_lib.SO)
    for s in ("gnngls_regret_labels", "gnngls_regret_labels_chunk"):
        assert hasattr(raw, s) and s in _lib.SIGNATURES
    assert lib.gnngls_abi_version() == 4
    assert lib.gnngls_regret_labels_chunk(2) == 0 and lib.gnngls_regret_labels_chunk(256) == 0
    assert lib.gnngls_regret_labels_chunk(100) == lib.gnngls_gls_resident_capacity(100)
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    call = lambda D, B, n, tour, iters, wd, out: lib.gnngls_regret_labels(D, B, n, tour, None, 30, iters, 0, wd, 0,  # noqa: E731
                                                                          out, out, out, out, out, None)
    hostile = [
        (None, 1, 20, p, 5, 1.0, p, b"NULL"),           # null pointers
        (p, 1, 20, None, 5, 1.0, p, b"NULL"),
        (p, 1, 20, p, 5, 1.0, None, b"NULL"),
        (p, -1, 20, p, 5, 1.0, p, b"NULL"),
        (p, 1, 2, p, 5, 1.0, p, b"n=2"),                # n < 3
        (p, 1, 256, p, 5, 1.0, p, b"n=256"),            # n > 255
        (p, 1, 20, p, -1, 1.0, p, b"max_outer_iters"),  # wall-clock mode is not a label
        (p, 1, 20, p, 5, 0.0, p, b"watchdog"),
    ]
    for D, B, n, tour, iters, wd, out, msg in hostile:
        assert call(D, B, n, tour, iters, wd, out) == -1
        assert b"regret_labels" in lib.gnngls_last_error() and msg in lib.gnngls_last_error()
    assert lib.gnngls_regret_labels(p, 1, 20, p, None, 30, 5, 7, 1.0, 0, p, p, p, p, p, None) == -1         # penalty_bits
    assert lib.gnngls_regret_labels(p, 1, 20, p, None, 30, 5, 0, 1.0, -3, p, p, p, p, p, None) == -1        # chunk_jobs
    assert lib.gnngls_regret_labels(None, 0, 20, None, None, 30, 5, 0, 1.0, 0, None, None, None, None, None, None) == 0


def test_labels_fail_cleanly_without_gpu(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from gnngls_amd import _lib, labels
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.gnngls_regret_labels(p, 1, 5, p, None, 30, 5, 0, 1.0, 0, p, p, p, p, p, None) == -2
    assert b"regret_labels" in lib.gnngls_last_error()
    D = np.zeros((1, 5, 5))
    with pytest.raises(_lib.GnnglsHipError):
        labels.regret_labels(D)
    G = nx.complete_graph(5)
    nx.set_edge_attributes(G, 1.0, "weight")
    from gnngls_amd import datasets, host
    with pytest.raises(_lib.GnnglsHipError):
        datasets.set_labels(G)
    with pytest.raises(_lib.GnnglsHipError):
        host.fixed_edge_tour(G, (1, 3))
