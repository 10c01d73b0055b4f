"""oracle/model_oracle.py -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

Plain PyTorch (CPU, fp32 or fp64) restatement of the reference's edge-regret GNN forward.
Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may import it.

Parity status
-------------
* Model wiring (gnngls/models.py:5-70): PINNED.  oracle/gen_golden.py executes the
  reference's own models.py verbatim (through the `dgl` shim in oracle/ref_import.py) and
  the golden outputs in tests/golden/model_*.npz come from that run;
  `EdgeRegretModelOracle` below is checked against them.
* dgl.nn.GATConv arithmetic (third party, dgl-cu111==0.6.1 pinned in Pipfile.lock:316-328,
  NOT in /root/reference, not installable offline): **parity unpinned**.  The reference holds
  no test or golden vector at that boundary.  `GATConvOracle` restates DGL 0.6.1's published
  algorithm (fc without bias -> el/er = sum(ft*attn) -> LeakyReLU(el[src]+er[dst], 0.2) ->
  softmax over the in-edges of each destination -> sum_src a*ft[src]); two independent
  formulations (edge-list scatter over networkx's own nx.line_graph, and a dense masked
  softmax built from the closed-form "share exactly one endpoint" rule) must agree
  (tests/test_model_oracle.py).  A third, `gat_aggregate_stars` on a `CompleteLineGraph`, uses neither an arc list nor
  networkx (dense blocks per star of K_n) and is what the GPU tests above n = 200 compare with; it is pinned to the
  edge-list form in the same file.

Graph convention: the GNN runs on the line graph of the complete TSP graph K_n
(gnngls/datasets.py:56-60).  Line-graph node id = rank of the TSP edge (i<j) in
itertools.combinations(range(n), 2) order -- the order generate_instances.py:31-33 inserts
edges in.
"""
import itertools
import math

import numpy as np
import torch
import torch.nn as nn


class LineGraph:
    """Minimal stand-in for the DGL graph object the reference passes around
    (datasets.py:56-60): line graph of K_n, node attribute 'e' = TSP edge of each node."""

    def __init__(self, n, src, dst, e):
        self.n = n
        self.src = src          # int64 [E]
        self.dst = dst          # int64 [E]
        self.ndata = {"e": e}   # int64 [N, 2]

    def number_of_nodes(self):
        return self.ndata["e"].shape[0]

    def to(self, device):
        return self


def edge_list(n):
    return list(itertools.combinations(range(n), 2))


def line_graph_closed_form(n):
    """Dense adjacency [N,N] (bool) from the rule: two TSP edges are adjacent iff they share
    exactly one endpoint (no self loops)."""
    e = np.array(edge_list(n), dtype=np.int64)
    a, b = e[:, 0], e[:, 1]
    share = (a[:, None] == a[None, :]).astype(np.int64) + (a[:, None] == b[None, :]) + \
            (b[:, None] == a[None, :]) + (b[:, None] == b[None, :])
    return torch.from_numpy(share == 1), torch.from_numpy(e)


def line_graph_networkx(n):
    """Edge list (src,dst) of the directed version of nx.line_graph(K_n), exactly as
    datasets.py:56-60 builds it (every undirected line-graph edge becomes two arcs,
    which is what dgl.from_networkx does for an undirected nx graph)."""
    import networkx as nx

    G = nx.Graph()
    G.add_nodes_from(range(n))
    for i, j in itertools.combinations(range(n), 2):
        G.add_edge(i, j)
    lG = nx.line_graph(G)
    rank = {e: r for r, e in enumerate(edge_list(n))}
    src, dst = [], []
    for u, v in lG.edges:
        ru, rv = rank[tuple(sorted(u))], rank[tuple(sorted(v))]
        src += [ru, rv]
        dst += [rv, ru]
    e = torch.tensor(edge_list(n), dtype=torch.int64)
    return LineGraph(n, torch.tensor(src, dtype=torch.int64), torch.tensor(dst, dtype=torch.int64), e)


def line_graph_arcs_closed_form(n):
    """The same directed arc set as line_graph_networkx(n), from the closed-form rule (destination {i,j} has the
    in-neighbours {i,k} and {k,j}, k not in {i,j}), as numpy index arithmetic -- networkx needs minutes and gigabytes for
    the 3.9 million undirected line-graph edges of K_200.  Arcs are sorted by destination (then source), which is what
    gat_aggregate_edge_list's chunked form needs.  tests/test_model_oracle.py checks the arc sets are equal for small n."""
    e = np.array(edge_list(n), dtype=np.int64)
    rank = np.full((n, n), -1, dtype=np.int64)
    rank[e[:, 0], e[:, 1]] = np.arange(len(e))
    rank[e[:, 1], e[:, 0]] = np.arange(len(e))
    i, j = e[:, 0], e[:, 1]
    k = np.arange(n)
    keep = (k[None, :] != i[:, None]) & (k[None, :] != j[:, None])          # [N, n]
    via_i = rank[i[:, None], k[None, :]]                                    # {i,k}
    via_j = rank[k[None, :], j[:, None]]                                    # {k,j}
    src = np.concatenate([via_i[keep].reshape(len(e), n - 2), via_j[keep].reshape(len(e), n - 2)], axis=1)
    src.sort(axis=1)
    dst = np.repeat(np.arange(len(e)), 2 * (n - 2))
    return LineGraph(n, torch.from_numpy(src.reshape(-1)), torch.from_numpy(dst), torch.from_numpy(e))


def batch_line_graphs(n, batch):
    """Disjoint union of `batch` copies of the line graph of K_n -- what dgl.batch (train.py:118-121) hands to the
    model: node ids of instance b are offset by b*N, arcs never cross instances."""
    g = line_graph_networkx(n)
    N = g.number_of_nodes()
    off = (torch.arange(batch, dtype=torch.int64) * N)[:, None]
    src = (g.src[None, :] + off).reshape(-1)
    dst = (g.dst[None, :] + off).reshape(-1)
    return LineGraph(n, src, dst, g.ndata["e"].repeat(batch, 1))


class CompleteLineGraph:
    """The line graph of K_n (or the disjoint union of `batch` copies of it) WITHOUT an arc list: what GATConvOracle needs to
    aggregate star by star (gat_aggregate_stars).  star[v] = line-graph ids of the n - 1 TSP edges at node v, by the other
    endpoint; with a batch, star[b * n + v] holds the ids of instance b (offset b * N).  Every line-graph node {i, j} sits in
    exactly two stars, i's and j's, and its in-neighbours are the other members of those two stars.
    block_elems: logits ([stars, H, n-1, n-1]) one group of stars may hold at a time."""

    def __init__(self, n, batch=1, block_elems=1 << 24):
        self.n, self.batch, self.block_elems = n, batch, block_elems
        e = np.array(edge_list(n), dtype=np.int64)
        N = len(e)
        rank = np.full((n, n), -1, dtype=np.int64)
        rank[e[:, 0], e[:, 1]] = np.arange(N)
        rank[e[:, 1], e[:, 0]] = np.arange(N)
        star = rank[~np.eye(n, dtype=bool)].reshape(n, n - 1)                 # row v: {v, k} for k != v, ascending k
        star = (star[None, :, :] + (np.arange(batch, dtype=np.int64) * N)[:, None, None]).reshape(batch * n, n - 1)
        self.star = torch.from_numpy(star)
        self.ndata = {"e": torch.from_numpy(e).repeat(batch, 1)}

    def number_of_nodes(self):
        return self.ndata["e"].shape[0]

    def to(self, device):
        return self


def complete_line_graph(n, batch=1):
    """The graph object of the large-n tests: same model outputs as line_graph_networkx(n) / batch_line_graphs(n, batch)
    (tests/test_model_oracle.py), at n = 257 in seconds and at n = 423 at all."""
    return CompleteLineGraph(n, batch)


def _star_logits(el, er, idx, slope):
    """[g, H, d, s] logits leaky_relu(el[s] + er[d]) over the stars idx [g, n-1]; s = d (a node is not its own in-neighbour)
    at -inf."""
    ns = idx.shape[1]
    a = el[idx].permute(0, 2, 1)[:, :, None, :]                              # [g, H, 1, s]
    b = er[idx].permute(0, 2, 1)[:, :, :, None]                              # [g, H, d, 1]
    e = torch.nn.functional.leaky_relu(a + b, slope)
    return e.masked_fill(torch.eye(ns, dtype=torch.bool), -math.inf)


def _star_block(ft, el, er, m, idx, slope):
    """One group of stars: per (star, destination, head) the sum of exp(e - m) over the star's other members and the same
    weights times ft -- the destination's softmax is the two stars' sums added (gat_aggregate_stars)."""
    p = torch.exp(_star_logits(el, er, idx, slope) - m[idx].permute(0, 2, 1)[:, :, :, None])     # [g, H, d, s]
    num = torch.matmul(p, ft[idx].permute(0, 2, 1, 3))                       # [g, H, d, s] x [g, H, s, F]
    return p.sum(dim=3).permute(0, 2, 1), num.permute(0, 2, 1, 3)            # [g, d, H], [g, d, H, F]


def gat_aggregate_stars(ft, el, er, graph, slope=0.2):
    """Formulation C, for the line graph of K_n only: destination {i, j} has the in-neighbours {i, k} and {k, j}, k not in
    {i, j} -- the other members of the star of i and of the star of j.  Per star the logits are a dense [n-1, n-1] block per
    head; a first pass takes every destination's maximum over both of its stars (detached: the softmax does not depend on the
    shift), a second accumulates exp(e - m), its sum and p @ ft[star] into the destinations by index_add.  No arc list and no
    [E, H, F] message tensor: n = 423 (75 million arcs) is 14 s per fp64 layer.  Under autograd every group of stars is a
    torch.utils.checkpoint segment, so a training step of n = 257 keeps one group's blocks alive at a time."""
    N, H, F = ft.shape
    star = graph.star
    ns = star.shape[1]
    assert N == graph.number_of_nodes() and ns >= 2
    g = max(1, graph.block_elems // (ns * ns * H))
    groups = [star[a:a + g] for a in range(0, star.shape[0], g)]
    with torch.no_grad():
        m = torch.full((N, H), -math.inf, dtype=ft.dtype)
        for idx in groups:
            part = _star_logits(el, er, idx, slope).amax(dim=3).permute(0, 2, 1)               # [g, d, H]
            m.scatter_reduce_(0, idx.reshape(-1, 1).expand(-1, H), part.reshape(-1, H), reduce="amax", include_self=True)
    ckpt = torch.is_grad_enabled() and (ft.requires_grad or el.requires_grad or er.requires_grad)
    z = torch.zeros((N, H), dtype=ft.dtype)
    out = torch.zeros((N, H, F), dtype=ft.dtype)
    for idx in groups:
        if ckpt:
            from torch.utils.checkpoint import checkpoint
            s, num = checkpoint(_star_block, ft, el, er, m, idx, slope, use_reentrant=False)
        else:
            s, num = _star_block(ft, el, er, m, idx, slope)
        z = z.index_add(0, idx.reshape(-1), s.reshape(-1, H))
        out = out.index_add(0, idx.reshape(-1), num.reshape(-1, H, F))
    return out / z[:, :, None]


class GATConvOracle(nn.Module):
    """dgl.nn.GATConv(in_feats, out_feats, num_heads) as called at gnngls/models.py:23, DGL 0.6.1
    defaults: feat_drop=attn_drop=0, negative_slope=0.2, residual=False, activation=None, no bias.
    State-dict keys: fc.weight [H*F, in], attn_l [1,H,F], attn_r [1,H,F]."""

    def __init__(self, in_feats, out_feats, num_heads, negative_slope=0.2, bias=False):
        super().__init__()
        # bias=True: DGL >= 0.7 (`rst = rst + bias.view(1, H, F)` after the aggregation); the pinned 0.6.1 has none
        self.bias = nn.Parameter(torch.zeros(num_heads * out_feats)) if bias else None
        self._num_heads = num_heads
        self._out_feats = out_feats
        self.negative_slope = negative_slope
        self.fc = nn.Linear(in_feats, out_feats * num_heads, bias=False)
        self.attn_l = nn.Parameter(torch.empty(1, num_heads, out_feats))
        self.attn_r = nn.Parameter(torch.empty(1, num_heads, out_feats))
        self.reset_parameters()

    def reset_parameters(self):
        gain = nn.init.calculate_gain("relu")
        nn.init.xavier_normal_(self.fc.weight, gain=gain)
        nn.init.xavier_normal_(self.attn_l, gain=gain)
        nn.init.xavier_normal_(self.attn_r, gain=gain)

    def forward(self, graph, feat):
        H, F = self._num_heads, self._out_feats
        ft = self.fc(feat).view(-1, H, F)
        el = (ft * self.attn_l).sum(dim=-1)                      # [N,H]
        er = (ft * self.attn_r).sum(dim=-1)                      # [N,H]
        if isinstance(graph, CompleteLineGraph):
            rst = gat_aggregate_stars(ft, el, er, graph, self.negative_slope)
        else:
            rst = gat_aggregate_edge_list(ft, el, er, graph.src, graph.dst, self.negative_slope)
        return rst if self.bias is None else rst + self.bias.view(1, H, F)


def gat_aggregate_edge_list(ft, el, er, src, dst, slope=0.2):
    """Formulation A: per-arc scores, scatter max / sum over destinations (what DGL's
    apply_edges(u_add_v) -> leaky_relu -> edge_softmax -> update_all(u_mul_e, sum) computes)."""
    N, H, F = ft.shape
    if src.numel() * H * F > _CHUNK_ELEMS:
        return _gat_aggregate_chunked(ft, el, er, src, dst, slope)
    e = torch.nn.functional.leaky_relu(el[src] + er[dst], slope)            # [E,H]
    idx = dst[:, None].expand(-1, H)
    m = torch.full((N, H), -math.inf, dtype=ft.dtype).scatter_reduce(0, idx, e, reduce="amax", include_self=True)
    p = torch.exp(e - m[dst])
    s = torch.zeros((N, H), dtype=ft.dtype).index_add_(0, dst, p)
    a = p / s[dst]
    out = torch.zeros((N, H, F), dtype=ft.dtype).index_add_(0, dst, a[:, :, None] * ft[src])
    return out


_CHUNK_ELEMS = 1 << 28       # [E,H,F] temporaries above this many elements (2 GiB in fp64) are built per destination range


def _gat_chunk(ft, el, er, s_, d_, d0, d1, slope):
    """gat_aggregate_edge_list restricted to the destinations d0 .. d1-1 (d_ = destination index - d0 of every arc)."""
    H, F = ft.shape[1], ft.shape[2]
    e = torch.nn.functional.leaky_relu(el[s_] + er[d0:d1][d_], slope)
    idx = d_[:, None].expand(-1, H)
    m = torch.full((d1 - d0, H), -math.inf, dtype=ft.dtype).scatter_reduce(0, idx, e.detach(), reduce="amax", include_self=True)
    p = torch.exp(e - m[d_])
    z = torch.zeros((d1 - d0, H), dtype=ft.dtype).index_add_(0, d_, p)
    w = p / z[d_]
    return torch.zeros((d1 - d0, H, F), dtype=ft.dtype).index_add_(0, d_, w[:, :, None] * ft[s_])


def _gat_aggregate_chunked(ft, el, er, src, dst, slope, arcs_per_chunk=1 << 20):
    """gat_aggregate_edge_list for graphs whose [E,H,F] message tensor does not fit in memory (K_200: 7.9 million arcs x
    128 features): the same formulas on consecutive destination ranges.  Arcs are brought into destination order first
    (stable: every destination's in-arcs keep their original order and sit in one range, so each range is the unchunked
    computation restricted to those destinations).  Under autograd every range is a torch.utils.checkpoint segment (its
    intermediates are recomputed in the backward instead of kept), so a training step of K_200 fits in a few GB.
    (The row maximum is detached here: the softmax does not depend on the shift; the one-shot form lets autograd carry that
    term, which cancels to rounding -- tests/test_model_oracle.py compares the gradients of the two forms.)"""
    N, H, F = ft.shape
    if not bool((dst[1:] >= dst[:-1]).all()):
        order = torch.sort(dst, stable=True).indices
        src, dst = src[order], dst[order]
    ckpt = torch.is_grad_enabled() and (ft.requires_grad or el.requires_grad or er.requires_grad)
    parts = []
    E, a = src.numel(), 0
    assert int(dst[0]) == 0 and int(dst[-1]) == N - 1
    while a < E:
        b = min(a + arcs_per_chunk, E)
        if b < E:                                                # extend to the end of the last destination's run
            b = int(torch.searchsorted(dst, dst[b - 1], right=True))
        d0, d1 = int(dst[a]), int(dst[b - 1]) + 1
        assert not parts or d0 == prev_d1                        # every node has in-arcs: the ranges tile 0 .. N-1
        s_, d_ = src[a:b], dst[a:b] - d0
        if ckpt:
            from torch.utils.checkpoint import checkpoint
            parts.append(checkpoint(_gat_chunk, ft, el, er, s_, d_, d0, d1, slope, use_reentrant=False))
        else:
            parts.append(_gat_chunk(ft, el, er, s_, d_, d0, d1, slope))
        prev_d1 = d1
        a = b
    return torch.cat(parts)


def gat_aggregate_dense(ft, el, er, adj, slope=0.2):
    """Formulation B: dense masked softmax; adj[d,s] True iff s is an in-neighbour of d."""
    e = torch.nn.functional.leaky_relu(el[None, :, :] + er[:, None, :], slope)   # [d,s,H]
    e = e.masked_fill(~adj[:, :, None], -math.inf)
    a = torch.softmax(e, dim=1)
    return torch.einsum("dsh,shf->dhf", a, ft)


class _Skip(nn.Module):
    """gnngls/models.py:5-15"""

    def __init__(self, module):
        super().__init__()
        self.module = module

    def forward(self, x, G=None):
        if G is not None:
            y = self.module(G, x).view(G.number_of_nodes(), -1)
        else:
            y = self.module(x)
        return x + y


class _AttentionLayer(nn.Module):
    """gnngls/models.py:18-41"""

    def __init__(self, embed_dim, n_heads, hidden_dim, gat_bias=False):
        super().__init__()
        self.message_passing = _Skip(GATConvOracle(embed_dim, embed_dim // n_heads, n_heads, bias=gat_bias))
        self.feed_forward = nn.Sequential(
            nn.BatchNorm1d(embed_dim),
            _Skip(nn.Sequential(nn.Linear(embed_dim, hidden_dim), nn.ReLU(), nn.Linear(hidden_dim, embed_dim))),
            nn.BatchNorm1d(embed_dim),
        )

    def forward(self, G, x):
        h = self.message_passing(x, G=G).view(G.number_of_nodes(), -1)
        return self.feed_forward(h)


class EdgeRegretModelOracle(nn.Module):
    """gnngls/models.py:44-70.  NOTE the layer count is `n_heads`, not `n_layers`
    (models.py:59-61 iterates range(n_heads)); hidden width 512 is hard-coded (models.py:60)."""

    def __init__(self, in_dim, embed_dim, out_dim, n_layers, n_heads=1, gat_bias=False):
        super().__init__()
        self.embed_dim = embed_dim
        self.embed_layer = nn.Linear(in_dim, embed_dim)
        self.message_passing_layers = nn.Sequential(
            *(_AttentionLayer(embed_dim, n_heads, 512, gat_bias) for _ in range(n_heads)))
        self.decision_layer = nn.Linear(embed_dim, out_dim)

    def forward(self, G, x):
        h = self.embed_layer(x)
        for l in self.message_passing_layers:
            h = l(G, h)
        return self.decision_layer(h)


def synthetic_state_dict(model, seed):
    """Seeded synthetic checkpoint (all data/ and models/ files in the reference tree are git-LFS
    pointer stubs).  Keeps the module's default initialisation and perturbs the BatchNorm running
    statistics and affine parameters so BatchNorm is not a no-op in eval mode."""
    g = torch.Generator().manual_seed(seed)
    sd = model.state_dict()
    out = {}
    for k, v in sd.items():
        if k.endswith("running_mean"):
            out[k] = 0.1 * torch.randn(v.shape, generator=g)
        elif k.endswith("running_var"):
            out[k] = 0.5 + torch.rand(v.shape, generator=g)
        elif k.endswith("num_batches_tracked"):
            out[k] = v.clone()
        elif ".feed_forward.0.weight" in k or ".feed_forward.2.weight" in k:
            out[k] = 1.0 + 0.1 * torch.randn(v.shape, generator=g)
        elif ".feed_forward.0.bias" in k or ".feed_forward.2.bias" in k:
            out[k] = 0.1 * torch.randn(v.shape, generator=g)
        else:
            out[k] = v.clone()
    return out


def trained_like_state_dict(model, seed, fc_gain=3.0, running_stats=None, calib_n=24):
    """A synthetic checkpoint with the weight scales a TRAINED model shows rather than those of the initialisation: BatchNorm
    gamma in [0.5, 4] and beta ~ N(0, 0.5), the GATConv linear map at `fc_gain` times its initial gain (larger attention logits),
    feed-forward weights at their default initialisation -- and, as in a trained model, the
    BatchNorm running statistics ARE the statistics of the activations (one calibration pass over a K_calib_n line graph with
    momentum 1), so the activations stay normalised from layer to layer instead of growing with gamma^16.
    running_stats: {key: tensor} of running_mean / running_var from an earlier calibration (the forward error fixtures store them:
    bit-identical checkpoints on every machine); None = calibrate here.  Returns (state_dict, running_stats).
    Such networks are ILL-CONDITIONED in fp32: a plain fp32 evaluation of the reference's own graph is 3 x (fc_gain 1) to 10-250 x
    (fc_gain 3) the 1e-5 parity bar away from the fp64 value at n = 50 -- the fixtures record that error next to the expected outputs."""
    g = torch.Generator().manual_seed(seed)
    sd = model.state_dict()
    out = {}
    for k, v in sd.items():
        if ".feed_forward.0.weight" in k or ".feed_forward.2.weight" in k:
            out[k] = 0.5 + 3.5 * torch.rand(v.shape, generator=g)          # gamma in [0.5, 4]
        elif ".feed_forward.0.bias" in k or ".feed_forward.2.bias" in k:
            out[k] = 0.5 * torch.randn(v.shape, generator=g)
        elif k.endswith("fc.weight"):
            out[k] = fc_gain * v.clone()
        else:
            out[k] = v.clone()
    if running_stats is None:
        import copy
        m = copy.deepcopy(model)
        m.load_state_dict(out)
        for mod in m.modules():
            if isinstance(mod, nn.BatchNorm1d):
                mod.momentum = 1.0
        m.train()
        N = calib_n * (calib_n - 1) // 2
        x = torch.rand((N, 1), generator=g)
        with torch.no_grad():
            m(line_graph_arcs_closed_form(calib_n), x)
        cal = m.state_dict()
        running_stats = {k: cal[k].clone() for k in cal if k.endswith("running_mean") or k.endswith("running_var")}
    for k, v in running_stats.items():
        out[k] = v.clone().to(out[k].dtype)
    return out, running_stats


def train_step_reference(model, G, x, target, criterion=None):
    """One optimisation step's forward/backward exactly as train.py:20-32 runs it (model.train(); y_pred = model(batch, x);
    loss = criterion(y_pred, y); loss.backward()), on CPU through torch autograd.
    -> (y_pred, loss, {param name: grad}, {buffer name: value after the step})."""
    criterion = criterion or nn.MSELoss()
    model.train()
    model.zero_grad()
    y = model(G, x)
    loss = criterion(y, target.type_as(y))
    loss.backward()
    grads = {k: p.grad.detach().clone() for k, p in model.named_parameters()}
    bufs = {k: b.detach().clone() for k, b in model.named_buffers()}
    return y.detach(), loss.detach(), grads, bufs


def minmax_transform(x, scale_, min_):
    """sklearn MinMaxScaler.transform: X * scale_ + min_ (datasets.py:85,88)."""
    return x * scale_ + min_


def minmax_inverse(y, scale_, min_):
    """sklearn MinMaxScaler.inverse_transform: (X - min_) / scale_ (test.py:79)."""
    return (y - min_) / scale_
