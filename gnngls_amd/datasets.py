"""Mirror of the input surface of gnngls/datasets.py (reference datasets.py:37-95): `TSPDataset` with
the same constructor, attributes (`instances`, `root_dir`, `scalers`, `G`) and `get_scaled_features`.

Differences forced by the environment, none on the arithmetic:
  * DGL is not needed: `self.G` / the returned graphs are `gnngls_amd.models.LineGraph` objects
    (the line graph of K_n has closed-form structure); `ndata` carries the same keys.
  * networkx >= 3 removed read_gpickle (datasets.py:56,69): instances are read with pickle.load.
  * git-LFS pointer stubs (every file under the reference's data/ and models/) are detected and
    reported instead of failing inside pickle.
`set_features` is kept; `set_labels` labels on the device (gnngls_amd.labels: fixed-edge searches instead of LKH).
"""
import pathlib
import pickle

import numpy as np
import torch

from .models import LineGraph

LFS_MAGIC = b"version https://git-lfs.github.com/spec/v1"


def is_lfs_pointer(path):
    with open(path, "rb") as f:
        return f.read(len(LFS_MAGIC)) == LFS_MAGIC


def read_gpickle(path):
    """nx.read_gpickle (datasets.py:56,69; gone in networkx 3) = pickle.load.  The reference's files were written by
    networkx 2.8 (Pipfile.lock): such a Graph unpickles under networkx 3.x with the views its generating code touched
    (`nodes`, `edges`, `adj`, `degree`: cached properties) in the instance dict and without the `__networkx_cache__` slot
    3.x creates in `Graph.__init__`; the slot is added here so the object is a complete 3.x graph (fixture:
    tests/golden/n3_tsp12/, tests/test_n3_ingestion_cpu.py)."""
    if is_lfs_pointer(path):
        raise FileNotFoundError(f"{path} is a git-LFS pointer stub, not the real object (fetch it with git lfs pull)")
    with open(path, "rb") as f:
        obj = pickle.load(f)
    if hasattr(obj, "_adj") and hasattr(obj, "_node") and "__networkx_cache__" not in getattr(obj, "__dict__", {}):
        obj.__dict__["__networkx_cache__"] = {}
    return obj


def set_features(G):
    """datasets.py:14-20"""
    for e in G.edges:
        G.edges[e]["features"] = np.array([G.edges[e]["weight"]], dtype=np.float32)


def _tour_from_edges(G, flag="in_solution"):
    """The tour from depot 0 through the edges flagged `flag`, or None if they do not form one Hamiltonian cycle."""
    n = len(G.nodes)
    adj = {v: [] for v in G.nodes}
    for i, j, d in G.edges(data=True):
        if d.get(flag):
            adj[i].append(j)
            adj[j].append(i)
    if any(len(a) != 2 for a in adj.values()):
        return None
    tour, prev = [0], None
    while len(tour) <= n:
        a, b = adj[tour[-1]]
        nxt = b if a == prev else a
        prev = tour[-1]
        tour.append(nxt)
        if nxt == 0:
            break
    return tour if len(tour) == n + 1 and tour[-1] == 0 and len(set(tour)) == n else None


def set_labels(G, **kwargs):
    """datasets.py:23-34 on the device: regret = (cost - base) / base for every edge, cost = the true cost of the fixed-edge
    search's tour (gnngls_amd.labels).  The base is G's `in_solution` tour when G has one (the reference's semantics:
    `optimal_cost(G)`), else the default base of labels.regret_labels.  If a search finds a tour cheaper than the base,
    `in_solution` is moved to the cheapest tour found, so that regret >= 0 and regret == 0 exactly on `in_solution`.
    kwargs go to labels.regret_labels.  Returns the labels.LabelResult of the instance."""
    from . import labels
    n = len(G.nodes)
    D = np.zeros((n, n), dtype=np.float64)
    for i, j, d in G.edges(data=True):
        D[i, j] = D[j, i] = d["weight"]
    base = _tour_from_edges(G) if all("in_solution" in d for _, _, d in G.edges(data=True)) else None
    res = labels.regret_labels(D[None], base_tour=None if base is None else [base], **kwargs)
    regret = res.regret[0].cpu().numpy()
    on = res.in_solution[0].cpu().numpy()
    for e in G.edges:
        r = labels.edge_rank(e[0], e[1], n)
        G.edges[e]["in_solution"] = bool(on[r])
        G.edges[e]["regret"] = 0. if on[r] else float(regret[r])
    return res


class TSPDataset(torch.utils.data.Dataset):
    def __init__(self, instances_file, scalers_file=None, feat_drop_idx=[]):
        if not isinstance(instances_file, pathlib.Path):
            instances_file = pathlib.Path(instances_file)
        self.root_dir = instances_file.parent
        if is_lfs_pointer(instances_file):
            raise FileNotFoundError(f"{instances_file} is a git-LFS pointer stub")
        self.instances = [line.strip() for line in open(instances_file)]

        if scalers_file is None:
            scalers_file = self.root_dir / "scalers.pkl"
        scalers = read_gpickle(scalers_file)
        if "edges" in scalers:  # for backward compatability (datasets.py:48-49)
            self.scalers = scalers["edges"]
        else:
            self.scalers = scalers

        self.feat_drop_idx = feat_drop_idx

        # only works for homogenous datasets (datasets.py:55-60)
        G = read_gpickle(self.root_dir / self.instances[0])
        self.G = LineGraph(len(G.nodes))

    def __len__(self):
        return len(self.instances)

    def __getitem__(self, i):
        if torch.is_tensor(i):
            i = i.tolist()
        G = read_gpickle(self.root_dir / self.instances[i])
        return self.get_scaled_features(G)

    def get_scaled_features(self, G):
        """datasets.py:73-95 (features / regret gathered in line-graph node order, MinMax-scaled)."""
        es = self.G.ndata["e"].numpy()
        features = np.vstack([G.edges[tuple(e)]["features"] for e in es])
        regret = np.vstack([G.edges[tuple(e)]["regret"] for e in es])
        features_transformed = self.scalers["features"].transform(features)
        features_transformed = np.delete(features_transformed, self.feat_drop_idx, axis=1)
        regret_transformed = self.scalers["regret"].transform(regret)

        H = LineGraph(self.G.n)
        H.ndata["features"] = torch.tensor(features_transformed, dtype=torch.float32)
        H.ndata["regret"] = torch.tensor(regret_transformed, dtype=torch.float32)
        H.ndata["in_solution"] = torch.tensor(regret, dtype=torch.float32)      # sic, datasets.py:94
        return H
