"""Regenerates tests/golden/pnn_law_n6.npz from the reference's own probabilistic_nearest_neighbour (algorithms.py:21-50).

    python tests/golden/make_pnn_fixtures.py        (needs the reference tree, see oracle/ref_import.py)

One symmetric 6-node instance with weights drawn from [1, 2]; the reference is called 20,000 times from depot 0 with
guide='weight', once with invert=True and once with invert=False, under np.random.seed(SEED).  The file holds arrays only: the
matrix, the depot, the 120 closed tours in itertools.permutations order and how often the reference returned each.  The instance
is accepted only if every tour's expected count under the definition (tests/test_sampling_cpu.tour_probability) is at least 5."""
import os
import sys

import networkx as nx
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle.ref_import import import_reference  # noqa: E402
from test_sampling_cpu import LAW_FIXTURE, all_tours, chi_square, chi_square_bound, tour_probability  # noqa: E402

N, DEPOT, CALLS, SEED = 6, 0, 20000, 20241


def main():
    ref = import_reference()
    rng = np.random.default_rng(SEED)
    upper = np.triu(rng.uniform(1.0, 2.0, size=(N, N)), 1)
    W = upper + upper.T
    G = nx.complete_graph(N)
    for i, j in G.edges:
        G.edges[i, j]["weight"] = W[i, j]
    tours = all_tours(N, DEPOT)
    index = {tuple(t): k for k, t in enumerate(tours)}
    out = {"W": W, "depot": DEPOT, "calls": CALLS, "seed": SEED, "tours": np.asarray(tours, dtype=np.int32)}
    np.random.seed(SEED)
    for name, invert in (("counts_invert", True), ("counts_plain", False)):
        counts = np.zeros(len(tours), dtype=np.int64)
        for _ in range(CALLS):
            counts[index[tuple(int(v) for v in ref.algorithms.probabilistic_nearest_neighbour(G, DEPOT, "weight", invert))]] += 1
        probs = np.array([tour_probability(W, t, invert) for t in tours])
        assert (probs * CALLS >= 5.0).all(), f"smallest expected count {probs.min() * CALLS:.2f} < 5: draw another instance"
        print(f"invert={invert}: smallest expected count {probs.min() * CALLS:.1f}, chi-square {chi_square(counts.astype(float), probs):.1f} "
              f"(bound {chi_square_bound(len(tours) - 1):.1f})")
        out[name] = counts
    np.savez(LAW_FIXTURE, **out)


if __name__ == "__main__":
    main()
