#!/usr/bin/env python
# coding: utf-8
"""Dataset split and feature scaling with the command line of the reference's scripts/preprocess_dataset.py
(preprocess_dataset.py:14-50): `preprocess_dataset.py dir [--n_train 100000] [--n_test 1000] [--n_val 10000]`, plus `--seed`
for the shuffle.  Writes train.txt, val.txt and test.txt (one instance path relative to `dir` per line) and scalers.pkl:
{'features': MinMaxScaler, 'regret': MinMaxScaler} fitted with partial_fit over the training instances.  Refuses an existing
scalers.pkl.  CPU only.

Differences: the instance list is sorted before the seeded shuffle (the reference shuffles glob order with the global
`random`, preprocess_dataset.py:27-28), and instances are read with pickle (networkx 3 has no read_gpickle).
"""
import argparse
import pathlib
import pickle
import random
import sys

import numpy as np
from sklearn.preprocessing import MinMaxScaler

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))

from gnngls_amd.datasets import read_gpickle  # noqa: E402


def main(argv=None):
    parser = argparse.ArgumentParser(description='Preprocess a dataset.')
    parser.add_argument('dir', type=pathlib.Path)
    parser.add_argument('--n_train', type=int, default=100000)
    parser.add_argument('--n_test', type=int, default=1000)
    parser.add_argument('--n_val', type=int, default=10000)
    parser.add_argument('--seed', type=int, default=None, help='seed of the shuffle')
    args = parser.parse_args(argv)

    if (args.dir / 'scalers.pkl').is_file():
        raise Exception('scalers.pkl already exists.')

    # train test split (preprocess_dataset.py:26-37)
    instances = sorted(p for p in args.dir.glob('*.pkl') if p.name != 'scalers.pkl')
    random.Random(args.seed).shuffle(instances)

    train_set = instances[:args.n_train]
    test_set = instances[args.n_train:args.n_train + args.n_test]
    val_set = instances[args.n_train + args.n_test:args.n_train + args.n_test + args.n_val]

    for data_set, file_name in zip([train_set, val_set, test_set], ['train.txt', 'val.txt', 'test.txt']):
        with open(args.dir / file_name, 'w') as data_file:
            for path in data_set:
                data_file.write(str(path.relative_to(args.dir)) + '\n')
            print(f'{file_name} contains {len(data_set)} instances.')

    scalers = {
        'features': MinMaxScaler(),
        'regret': MinMaxScaler()
    }
    for instance_path in train_set:
        G = read_gpickle(instance_path)
        for k in scalers:
            scalers[k].partial_fit(np.vstack([G.edges[e][k] for e in G.edges]))

    with open(args.dir / 'scalers.pkl', 'wb') as f:
        pickle.dump(scalers, f)


if __name__ == '__main__':
    main()
