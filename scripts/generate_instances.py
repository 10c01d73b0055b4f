#!/usr/bin/env python
# coding: utf-8
"""Dataset generation with the command line of the reference's scripts/generate_instances.py (generate_instances.py:43-47):
`generate_instances.py n_samples n_nodes dir`, plus `--seed`, `--batch_size`, `--solve_iters`, `--label_iters`,
`--perturbation_moves` and `--use_gpu`.  It refuses an existing `dir`.

Instances follow generate_instances.py:25-33: uniform points in the unit square (node attribute `pos`), edges added in
itertools.combinations order with `weight` = np.linalg.norm(pos[j] - pos[i]) (np.float64).  Each is written as one pickled
networkx Graph `<32 hex digits>.pkl` (uuid-shaped names drawn from the seeded generator, generate_instances.py:57) with
`in_solution` (bool), `features` (float32[1], datasets.py:14-20) and `regret` (float, datasets.py:23-34).

What differs is the labelling: Concorde's optimum and LKH's fixed-edge tours are replaced by the fixed-edge searches of
gnngls_amd.labels, a batch of instances at a time on the MI355X (`in_solution` = the best tour found, not a proven optimum).
There is no CPU path: `--use_gpu` is required.  Pickling runs on the host.
"""
import argparse
import itertools
import pathlib
import pickle
import sys

import networkx as nx
import numpy as np

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))

from gnngls_amd import datasets, labels  # noqa: E402


def make_instance(rng, n_nodes):
    """generate_instances.py:25-33 with a seeded generator."""
    G = nx.Graph()
    coords = rng.random((n_nodes, 2))
    for v, p in enumerate(coords):
        G.add_node(v, pos=p)
    for i, j in itertools.combinations(G.nodes, 2):
        G.add_edge(i, j, weight=np.linalg.norm(G.nodes[j]['pos'] - G.nodes[i]['pos']))
    return G


def weight_matrix(G):
    n = len(G.nodes)
    D = np.zeros((n, n), dtype=np.float64)
    for i, j, d in G.edges(data=True):
        D[i, j] = D[j, i] = d['weight']
    return D


def main(argv=None):
    parser = argparse.ArgumentParser(description='Generate a dataset.')
    parser.add_argument('n_samples', type=int)
    parser.add_argument('n_nodes', type=int)
    parser.add_argument('dir', type=pathlib.Path)
    parser.add_argument('--seed', type=int, default=None, help='seed of the instance and file-name generator')
    parser.add_argument('--batch_size', type=int, default=64, help='instances labelled per device call')
    parser.add_argument('--solve_iters', type=int, default=labels.SOLVE_ITERS, help='outer iterations of the base search')
    parser.add_argument('--label_iters', type=int, default=labels.LABEL_ITERS, help='outer iterations per fixed-edge search')
    parser.add_argument('--perturbation_moves', type=int, default=labels.PERTURBATION_MOVES)
    parser.add_argument('--use_gpu', action='store_true')
    args = parser.parse_args(argv)

    if not args.use_gpu:
        parser.error('labels are generated on the GPU only (fixed-edge searches on the MI355X): pass --use_gpu')
    if args.dir.exists():
        raise Exception(f'Output directory {args.dir} exists.')
    if args.n_samples < 0 or args.n_nodes < 3 or args.batch_size < 1:
        parser.error('n_samples >= 0, n_nodes >= 3 and batch_size >= 1 required')
    args.dir.mkdir(parents=True)

    rng = np.random.default_rng(args.seed)
    written = unsettled = 0
    while written < args.n_samples:
        b = min(args.batch_size, args.n_samples - written)
        graphs = [make_instance(rng, args.n_nodes) for _ in range(b)]
        res = labels.regret_labels(np.stack([weight_matrix(G) for G in graphs]), solve_iters=args.solve_iters,
                                   label_iters=args.label_iters, perturbation_moves=args.perturbation_moves)
        status = res.status.cpu().numpy()
        bad = np.isin(status, [labels.STATUS_WATCHDOG, labels.STATUS_EDGE_LOST])
        if bad.any():
            raise RuntimeError(f'fixed-edge searches failed: status {status[bad].tolist()}')
        unsettled += int((status == labels.STATUS_UNSETTLED).sum())
        regret = res.regret.cpu().numpy()
        on = res.in_solution.cpu().numpy()
        for k, G in enumerate(graphs):
            # edges were added in combinations order: edge number r is line-graph node r
            for r, e in enumerate(G.edges):
                G.edges[e]['in_solution'] = bool(on[k, r])
            datasets.set_features(G)
            for r, e in enumerate(G.edges):
                G.edges[e]['regret'] = 0. if on[k, r] else float(regret[k, r])
            with open(args.dir / f'{rng.bytes(16).hex()}.pkl', 'wb') as f:
                pickle.dump(G, f, protocol=pickle.HIGHEST_PROTOCOL)
        written += b
        print(f'{written}/{args.n_samples} instances', flush=True)
    if unsettled:
        print(f'warning: {unsettled} instances still improved their base after the last repair round', file=sys.stderr)


if __name__ == '__main__':
    main()
