"""CPU checks of oracle/model_oracle.py: (a) the two independent GATConv formulations agree,
(b) the oracle's own wiring reproduces the golden outputs captured from the reference's models.py
(run verbatim through the dgl shim), (c) the MinMax scaler restatement matches sklearn's fp32 results, (d) the star form of the aggregation that the GPU tests above
n = 200 use (complete_line_graph) is the edge-list form on networkx's line graph: values, gradients, the whole model."""
import os

import numpy as np
import pytest
import torch

from oracle import model_oracle as mo

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.mark.parametrize("n", [4, 5, 9])
def test_gat_formulations_agree(n):
    torch.manual_seed(n)
    G = mo.line_graph_networkx(n)
    adj, e = mo.line_graph_closed_form(n)
    N = G.number_of_nodes()
    assert N == n * (n - 1) // 2 and torch.equal(e, G.ndata["e"])
    # in-degree 2(n-2), no self loops (datasets.py:56-60)
    assert torch.equal(adj.sum(1), torch.full((N,), 2 * (n - 2)))
    assert len(G.src) == N * 2 * (n - 2)
    dense_from_edges = torch.zeros((N, N), dtype=torch.bool)
    dense_from_edges[G.dst, G.src] = True
    assert torch.equal(dense_from_edges, adj)
    ft = torch.randn(N, 8, 16, dtype=torch.float64)
    el = torch.randn(N, 8, dtype=torch.float64) * 3
    er = torch.randn(N, 8, dtype=torch.float64) * 3
    a = mo.gat_aggregate_edge_list(ft, el, er, G.src, G.dst)
    b = mo.gat_aggregate_dense(ft, el, er, adj)
    assert torch.allclose(a, b, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("n", [4, 7, 13])
def test_closed_form_arcs_and_chunked_aggregation(n):
    """The arc list the large-n GPU tests use (closed-form rule, sorted by destination) is networkx's own line graph,
    and the destination-range form of the aggregation gives the same bits as the one-shot form."""
    torch.manual_seed(100 + n)
    G, C = mo.line_graph_networkx(n), mo.line_graph_arcs_closed_form(n)
    assert sorted(zip(G.dst.tolist(), G.src.tolist())) == list(zip(C.dst.tolist(), C.src.tolist()))   # sorted by (dst, src)
    assert torch.equal(C.ndata["e"], G.ndata["e"])
    N = C.number_of_nodes()
    ft = torch.randn(N, 8, 16, dtype=torch.float64)
    el, er = torch.randn(N, 8, dtype=torch.float64) * 3, torch.randn(N, 8, dtype=torch.float64) * 3
    whole = mo.gat_aggregate_edge_list(ft, el, er, C.src, C.dst)
    parts = mo._gat_aggregate_chunked(ft, el, er, C.src, C.dst, 0.2, arcs_per_chunk=41)
    assert torch.equal(whole, parts)
    assert torch.allclose(whole, mo.gat_aggregate_edge_list(ft, el, er, G.src, G.dst), rtol=1e-13, atol=1e-13)
    # arcs in networkx's own (unsorted) order: brought into destination order first, same bits as the one-shot form
    assert torch.equal(mo._gat_aggregate_chunked(ft, el, er, G.src, G.dst, 0.2, arcs_per_chunk=29),
                       mo.gat_aggregate_edge_list(ft, el, er, G.src, G.dst))


def test_chunked_aggregation_gradients_match_the_one_shot_form():
    """Under autograd the destination-range form (checkpointed ranges, what the TSP200 training test differentiates) gives
    the gradients of the one-shot form."""
    torch.manual_seed(3)
    C = mo.line_graph_arcs_closed_form(8)
    N = C.number_of_nodes()
    leaves = [torch.randn(N, 8, 16, dtype=torch.float64, requires_grad=True),
              torch.randn(N, 8, dtype=torch.float64, requires_grad=True), torch.randn(N, 8, dtype=torch.float64, requires_grad=True)]
    wgt = torch.randn(N, 8, 16, dtype=torch.float64)
    ga = torch.autograd.grad((mo.gat_aggregate_edge_list(*leaves, C.src, C.dst) * wgt).sum(), leaves)
    gb = torch.autograd.grad((mo._gat_aggregate_chunked(*leaves, C.src, C.dst, 0.2, arcs_per_chunk=50) * wgt).sum(), leaves)
    for x, y in zip(ga, gb):
        assert torch.allclose(x, y, rtol=1e-11, atol=1e-12)


EPS64 = float(np.finfo(np.float64).eps)


def star_inputs(N, H, seed):
    g = torch.Generator().manual_seed(seed)
    ft = torch.randn(N, H, 128 // H, dtype=torch.float64, generator=g)
    el = torch.randn(N, H, dtype=torch.float64, generator=g) * 3
    er = torch.randn(N, H, dtype=torch.float64, generator=g) * 3
    return ft, el, er


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("H", [1, 2, 4, 8, 16])
@pytest.mark.parametrize("n", [3, 4, 5, 12, 30])
def test_star_aggregation_equals_the_edge_list_form(n, H, B):
    """The block form the GPU tests above n = 200 rest on (gat_aggregate_stars: dense logits per star of K_n, no arc list) is
    the edge-list form on networkx's own line graph, for every head count and for a batch of disjoint instances.  Both
    normalise a sum of up to 2 (n - 2) = 56 terms of magnitude <= 1 in a different order, in fp64: the bar is 64 eps of the
    largest output (1.4e-14 relative).  Measured over all 50 cases, several groups of stars per case: at worst 5.3e-15 on
    outputs up to 2.95, i.e. 8 eps."""
    G, C = mo.batch_line_graphs(n, B), mo.complete_line_graph(n, B)
    C.block_elems = 5000                                             # n = 12: 41 logits per (star, head) ... several groups
    N = G.number_of_nodes()
    assert C.number_of_nodes() == N == B * n * (n - 1) // 2 and torch.equal(C.ndata["e"], G.ndata["e"])
    # every node in exactly two stars, no star across instances
    assert torch.equal(torch.bincount(C.star.reshape(-1), minlength=N), torch.full((N,), 2))
    assert torch.equal(C.star // (N // B), (torch.arange(B * n) // n)[:, None].expand(-1, n - 1))
    ft, el, er = star_inputs(N, H, 1000 * n + 10 * H + B)
    a = mo.gat_aggregate_edge_list(ft, el, er, G.src, G.dst)
    b = mo.gat_aggregate_stars(ft, el, er, C)
    assert a.shape == b.shape == (N, H, 128 // H)
    worst = (a - b).abs().max().item()
    print(f"star vs edge-list n={n} H={H} B={B}: {worst:.1e} on outputs up to {a.abs().max().item():.2f}")
    assert worst <= 64 * EPS64 * a.abs().max().item(), (worst, a.abs().max().item())


@pytest.mark.parametrize("H", [8, 2])
@pytest.mark.parametrize("n", [5, 12])
def test_star_aggregation_gradients_match_the_one_shot_form(n, H):
    """Under autograd (checkpointed groups of stars, detached maximum) the block form gives the gradients of the one-shot
    edge-list form with respect to ft, el and er; tolerance of test_chunked_aggregation_gradients_match_the_one_shot_form."""
    G, C = mo.line_graph_networkx(n), mo.complete_line_graph(n)
    C.block_elems = 3 * (n - 1) * (n - 1) * H                        # three stars per checkpoint segment
    N = G.number_of_nodes()
    leaves = [t.requires_grad_() for t in star_inputs(N, H, 7 * n + H)]
    wgt = torch.randn(N, H, 128 // H, dtype=torch.float64, generator=torch.Generator().manual_seed(n))
    ga = torch.autograd.grad((mo.gat_aggregate_edge_list(*leaves, G.src, G.dst) * wgt).sum(), leaves)
    gb = torch.autograd.grad((mo.gat_aggregate_stars(*leaves, C) * wgt).sum(), leaves)
    for x, y in zip(ga, gb):
        assert torch.allclose(x, y, rtol=1e-11, atol=1e-12)


def init_scale_oracle(dtype=torch.float64):
    """The oracle half of tests/test_model_gpu.py's make_models() (same seeds; that one also builds the HIP model on a GPU)."""
    torch.manual_seed(1234)
    oracle = mo.EdgeRegretModelOracle(1, 128, 1, 3, n_heads=8)
    oracle.load_state_dict(mo.synthetic_state_dict(oracle, seed=99))
    return oracle.to(dtype)


def test_whole_model_on_the_star_graph_equals_the_networkx_graph():
    """EdgeRegretModelOracle (8 layers, fp64) on complete_line_graph(8, 2) against the same model on batch_line_graphs(8, 2):
    eval-mode outputs, and a training step through train_step_reference -- predictions, loss, every gradient and the
    BatchNorm running statistics (BatchNorm sees all B * N rows, the aggregation stays per instance).  The two aggregations
    differ by ~10 eps per layer and the network amplifies a perturbation by ~1e2 (its fp32 evaluation sits at 1e-5 with
    eps 6e-8): bar 1e-11 of each tensor's largest entry.  Measured: eval outputs 2.3e-15, training predictions 1.1e-14, loss
    1.5e-15, gradients <= 3.1e-13 (embed_layer.bias), running statistics <= 6e-15 of it."""
    import copy
    n, B = 8, 2
    G, C = mo.batch_line_graphs(n, B), mo.complete_line_graph(n, B)
    C.block_elems = 5 * (n - 1) * (n - 1) * 8
    N = G.number_of_nodes()
    rng = np.random.default_rng(8)
    x = torch.from_numpy(rng.random((N, 1)))
    target = torch.from_numpy(rng.random((N, 1)))

    measured = {}

    def close(a, b, what):
        scale = b.abs().max().item()
        worst = (a - b).abs().max().item()
        measured[what] = worst / max(scale, 1e-300)
        assert worst <= 1e-11 * scale + 1e-300, (what, worst, scale)

    model = init_scale_oracle().eval()
    with torch.no_grad():
        close(model(C, x), model(G, x), "eval")
    ya, la, ga, ba = mo.train_step_reference(copy.deepcopy(model), G, x, target)
    yb, lb, gb, bb = mo.train_step_reference(copy.deepcopy(model), C, x, target)
    close(yb, ya, "train y")
    close(lb, la, "loss")
    gmax = max(v.abs().max().item() for v in ga.values())
    assert set(ga) == set(gb) and set(ba) == set(bb)
    for k in ga:
        if ga[k].abs().max().item() <= 1e-9 * gmax:           # a Linear bias feeding a BatchNorm: zero up to rounding in both
            assert gb[k].abs().max().item() <= 1e-9 * gmax, k
        else:
            close(gb[k], ga[k], k)
    for k in ba:
        if ba[k].dtype.is_floating_point:
            close(bb[k], ba[k], k)
        else:
            assert torch.equal(bb[k], ba[k]), k
    print("star graph vs networkx graph, worst |difference| / largest entry: " + ", ".join(
        f"{k} {v:.1e}" for k, v in sorted(measured.items(), key=lambda kv: -kv[1])[:4]))


def test_forward_bar_catches_one_dropped_source_at_n117():
    """Teeth of tests/test_model_edges_gpu.py: at n = 117 (first size of the head-split gat_rows) every destination loses ONE
    of its 230 in-neighbours -- what a tile-edge off-by-one does.  The softmax loses about 1/230 of its weight, and the fp64
    one-layer output at initialisation-scale weights moves by far more than the forward bar 1e-5 * max(|ref|, max|ref|).
    Measured: |moved| / bar is 65 at the worst output and 16 at the median one; the intact arc list reproduces the star form
    to 1e-11 of the largest output (asserted)."""
    from test_model_gpu import regret_bound
    n = 117
    N = n * (n - 1) // 2
    model = init_scale_oracle().eval()
    model.message_passing_layers = model.message_passing_layers[:1]
    x = torch.from_numpy(np.random.default_rng(n).random((N, 1)))
    A = mo.line_graph_arcs_closed_form(n)
    deg = 2 * (n - 2)
    keep = torch.arange(len(A.src)) % deg != deg - 1                 # arcs are sorted by destination: drop the last of each
    D = mo.LineGraph(n, A.src[keep], A.dst[keep], A.ndata["e"])
    assert torch.equal(torch.bincount(D.dst, minlength=N), torch.full((N,), deg - 1))
    with torch.no_grad():
        ref = model(mo.complete_line_graph(n), x).numpy().reshape(-1)
        full = model(A, x).numpy().reshape(-1)
        dropped = model(D, x).numpy().reshape(-1)
    assert np.abs(full - ref).max() <= 1e-11 * np.abs(ref).max()
    ratio = np.abs(dropped - ref) / regret_bound(ref)
    print(f"n=117, one source dropped per destination: |moved| / bar worst {ratio.max():.1f}, median {np.median(ratio):.2f}")
    assert ratio.max() > 1.0


def build_oracle_model():
    g = np.load(os.path.join(GOLD, "model_n5.npz"))
    torch.manual_seed(int(g["model_seed"]))
    model = mo.EdgeRegretModelOracle(1, 128, 1, 3, n_heads=8)
    sd = mo.synthetic_state_dict(model, seed=int(g["sd_seed"]))
    model.load_state_dict(sd)
    model.eval()
    checksum = float(sum(v.double().abs().sum() for v in sd.values() if v.dtype.is_floating_point))
    assert checksum == float(g["sd_checksum"]), "torch RNG stream differs from the one the goldens were made with"
    assert sum(p.numel() for p in model.parameters()) == int(g["n_params"]) == 1191297
    return model


def test_state_dict_layout():
    model = build_oracle_model()
    keys = set(model.state_dict().keys())
    assert len(model.message_passing_layers) == 8          # models.py:59-61: n_heads layers
    for k in ("embed_layer.weight", "decision_layer.bias",
              "message_passing_layers.7.message_passing.module.fc.weight",
              "message_passing_layers.0.message_passing.module.attn_l",
              "message_passing_layers.0.feed_forward.0.running_mean",
              "message_passing_layers.0.feed_forward.1.module.0.weight",
              "message_passing_layers.0.feed_forward.1.module.2.bias",
              "message_passing_layers.0.feed_forward.2.running_var"):
        assert k in keys


@pytest.mark.parametrize("n", [5, 10, 20])
def test_model_matches_reference_wiring(n):
    model = build_oracle_model()
    g = np.load(os.path.join(GOLD, f"model_n{n}.npz"))
    G = mo.line_graph_networkx(n)
    with torch.no_grad():
        y = model(G, torch.from_numpy(g["x"]))
    assert np.array_equal(y.numpy(), g["y"])      # same ops in the same order: bitwise


def test_minmax_scaler_fp32():
    g = np.load(os.path.join(GOLD, "misc.npz"))
    s, m = g["scaler_scale"], g["scaler_min"]
    # sklearn: X(float32) *= scale_(float64) ; X += min_   -> fp64 arithmetic, rounded to fp32 twice
    fwd = (g["scaler_in"].astype(np.float64) * s).astype(np.float32)
    fwd = (fwd.astype(np.float64) + m).astype(np.float32)
    assert np.array_equal(fwd, g["scaler_fwd"])
    inv = (g["scaler_inv_in"].astype(np.float64) - m).astype(np.float32)
    inv = (inv.astype(np.float64) / s).astype(np.float32)
    assert np.array_equal(inv, g["scaler_inv"])


@pytest.mark.parametrize("n", [5, 8])
def test_train_step_matches_reference_golden(n):
    """One training step (train.py:20-32) of the oracle's own wiring vs the fixture captured from the reference's
    models.py: predictions, loss, every parameter gradient (sum, abs-sum, strided sample) and the BatchNorm running
    statistics after the step."""
    g = np.load(os.path.join(GOLD, f"train_n{n}.npz"))
    torch.manual_seed(int(g["model_seed"]))
    model = mo.EdgeRegretModelOracle(1, 128, 1, 3, n_heads=8)
    model.load_state_dict(mo.synthetic_state_dict(model, seed=int(g["sd_seed"])))
    G = mo.batch_line_graphs(n, int(g["batch"]))
    y, loss, grads, bufs = mo.train_step_reference(model, G, torch.from_numpy(g["x"]), torch.from_numpy(g["target"]))
    # same torch ops in the same wiring, but CPU scatter/GEMM reductions are multi-threaded: fp32 reordering noise, and now
    # and then a ReLU / LeakyReLU pre-activation within rounding distance of 0 takes the other branch and moves a few
    # gradient rows by ~1e-3 of the tensor's largest entry -> typical (median) agreement tight, worst case loose
    assert np.allclose(y.numpy(), g["y"], rtol=1e-5, atol=1e-6) and abs(loss.item() - g["loss"]) <= 1e-6 * g["loss"]
    rels = []
    for k, gr in grads.items():
        flat = gr.double().reshape(-1).numpy()
        top = np.abs(g["gval/" + k]).max()
        if top < 1e-6:                       # a Linear bias feeding a BatchNorm: exactly zero gradient, stored noise
            assert np.abs(flat).max() < 1e-6, k
            continue
        rels.append(np.abs(flat[g["gidx/" + k]] - g["gval/" + k]).max() / top)
        assert abs(np.abs(flat).sum() - g["gabs/" + k]) <= 5e-3 * g["gabs/" + k], k
    assert np.median(rels) <= 5e-5 and max(rels) <= 5e-3, (np.median(rels), max(rels))
    for k, b in bufs.items():
        assert np.allclose(b.numpy(), g["buf/" + k], rtol=1e-5, atol=1e-7), k


def test_batched_line_graph_is_disjoint_union():
    n, B = 6, 3
    G1, GB = mo.line_graph_networkx(n), mo.batch_line_graphs(n, B)
    N = G1.number_of_nodes()
    assert GB.number_of_nodes() == B * N and len(GB.src) == B * len(G1.src)
    assert torch.equal(GB.src // N, GB.dst // N)                      # no arc crosses instances
    assert torch.equal(GB.src[:len(G1.src)], G1.src) and torch.equal(GB.dst[-len(G1.dst):] - (B - 1) * N, G1.dst)
