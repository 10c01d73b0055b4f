"""Regenerates tests/golden/insertion_*.npz from the reference's own insertion / cheapest_insertion (algorithms.py:67-108).

    python tests/golden/make_insertion_fixtures.py        (needs the reference tree, see oracle/ref_import.py)

The files hold arrays only: the fp64 matrices (one per instance, shared by its cases), depot, mode (index into
test_insertion_cpu.MODES), the reference's tour and, for mode 'random', the seed given to np.random.seed before the call and
the value of np.random.random() drawn right after the reference returned.  insertion_steps.npz holds single
cheapest_insertion steps on arbitrary closed sub-tours with the reference's tour_cost of the result."""
import os
import sys

import networkx as nx
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle.ref_import import import_reference  # noqa: E402
from test_insertion_cpu import GOLDEN, MODES, make_instance  # noqa: E402


def graph_of(D):
    G = nx.complete_graph(D.shape[0])
    for i, j in G.edges:
        G.edges[i, j]["weight"] = D[i, j]
    return G


def whole_constructions(ref, instances, rng):
    out = {"n_cases": 0}
    c = 0
    for k, D in enumerate(instances):
        n = D.shape[0]
        out[f"D{k}"] = D
        G = graph_of(D)
        depots = [0, n - 1] if n <= 3 else [0, int(rng.integers(1, n))]
        for depot in depots:
            for m, mode in enumerate(MODES):
                seed = int(rng.integers(0, 2 ** 31 - 1))
                np.random.seed(seed)
                tour = ref.algorithms.insertion(G, depot, mode=mode)
                nxt = np.random.random()
                out[f"c{c}_inst"], out[f"c{c}_depot"], out[f"c{c}_mode"] = k, depot, m
                out[f"c{c}_tour"] = np.asarray(tour, dtype=np.int32)
                out[f"c{c}_seed"], out[f"c{c}_next"] = seed, nxt
                c += 1
    out["n_cases"] = c
    return out


def single_steps(ref, instances, rng):
    out = {"n_cases": 0}
    c = 0
    for k, D in enumerate(instances):
        n = D.shape[0]
        out[f"D{k}"] = D
        G = graph_of(D)
        for m in sorted({0, 1, 2, n // 2, n - 2}):
            if m < 0 or m > n - 2:
                continue
            perm = rng.permutation(n)
            d, inner, v = int(perm[0]), perm[1:1 + m].tolist(), int(perm[1 + m])
            sub = [d] + [int(x) for x in inner] + [d]
            tour = ref.algorithms.cheapest_insertion(G, sub, v)
            out[f"c{c}_inst"], out[f"c{c}_sub"], out[f"c{c}_node"] = k, np.asarray(sub, dtype=np.int32), v
            out[f"c{c}_tour"] = np.asarray(tour, dtype=np.int32)
            out[f"c{c}_cost"] = np.float64(ref.tour_cost(G, tour))
            c += 1
    out["n_cases"] = c
    return out


def main():
    ref = import_reference()
    rng = np.random.default_rng(20261016)
    euclid = [make_instance("euclid", n, rng) for n in (2, 3, 5, 8, 20, 50, 100, 200)]
    ties = [make_instance(kind, n, rng) for kind in ("grid", "lattice", "noise") for n in (5, 12, 30, 64)]
    np.savez_compressed(os.path.join(GOLDEN, "insertion_euclid.npz"), **whole_constructions(ref, euclid, rng))
    np.savez_compressed(os.path.join(GOLDEN, "insertion_ties.npz"), **whole_constructions(ref, ties, rng))
    steps = [make_instance(kind, n, rng) for kind, n in (("euclid", 4), ("euclid", 31), ("grid", 12), ("lattice", 40),
                                                        ("noise", 24), ("euclid", 90))]
    np.savez_compressed(os.path.join(GOLDEN, "insertion_steps.npz"), **single_steps(ref, steps, rng))
    for name in ("insertion_euclid.npz", "insertion_ties.npz", "insertion_steps.npz"):
        print(name, os.path.getsize(os.path.join(GOLDEN, name)), "bytes")


if __name__ == "__main__":
    main()
