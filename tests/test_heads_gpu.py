"""Head counts other than 8 (embed_dim 128: H in {1, 2, 4, 16}, F = 128 / H features per head, H layers as in the reference,
models.py:59-61) on the MI355X: inference forward (fp32 and prepared paths), training step, torch op and the train.py /
test.py command line, against the CPU oracle of the same architecture (oracle/model_oracle.py)."""
import copy
import os

import numpy as np
import pytest
import torch

from test_train_gpu import gradient_error_metrics, gradient_errors_acceptable

pytestmark = pytest.mark.gpu

HEADS = [1, 2, 4, 16]
RTOL = 1e-5


def regret_bound(ref):
    ref = np.abs(np.asarray(ref, dtype=np.float64))
    return RTOL * np.maximum(ref, ref.max())


def make_models(H, in_dim=1, seed=1234, sd_seed=99, gat_bias=False, trained_like=False):
    from gnngls_amd.models import EdgePropertyPredictionModel
    from oracle import model_oracle as mo
    torch.manual_seed(seed)
    oracle = mo.EdgeRegretModelOracle(in_dim, 128, 1, 3, n_heads=H, gat_bias=gat_bias)
    if trained_like:
        sd, _ = mo.trained_like_state_dict(oracle, seed=sd_seed, calib_n=12)
    else:
        sd = mo.synthetic_state_dict(oracle, seed=sd_seed)
    if gat_bias:
        gen = torch.Generator().manual_seed(sd_seed + 1)
        for k in list(sd):
            if k.endswith("message_passing.module.bias"):
                sd[k] = 0.3 * torch.randn(sd[k].shape, generator=gen)
    oracle.load_state_dict(sd)
    model = EdgePropertyPredictionModel(in_dim, 128, 1, 3, n_heads=H)
    res = model.load_state_dict(sd)
    assert not res.missing_keys and not res.unexpected_keys
    assert len(model.message_passing_layers) == H
    return model.to("cuda"), oracle, sd


def forward_both(model, x, B, n):
    """The prepared (bf16x3 feed-forward) path of models.regret_forward and the fp32 path of the one-call entry."""
    from gnngls_amd import _lib
    from gnngls_amd import models as M
    import ctypes
    y_prep = M.regret_forward(model, x, B, n)
    L = _lib.load()
    N = n * (n - 1) // 2
    packed = model.pack_weights("cuda")
    ws = torch.empty(int(L.gnngls_regret_forward_workspace_bytes_heads(B, n, model.n_heads)), dtype=torch.uint8, device="cuda")
    y32 = torch.empty((B, N), dtype=torch.float32, device="cuda")
    _lib.check(L.gnngls_regret_forward_prepared_heads(_lib.ptr(x), _lib.ptr(packed), None, 0, B, n, model.in_dim,
                                                      len(model.message_passing_layers), model.n_heads, _lib.ptr(y32), _lib.ptr(ws),
                                                      ctypes.c_int64(ws.numel()), _lib.current_stream()), "regret_forward")
    return y_prep, y32


def check_forward(model, oracle, n, B, in_dim, seed, graph=None):
    from oracle import model_oracle as mo
    model.eval()
    N = n * (n - 1) // 2
    x = torch.from_numpy(np.random.default_rng(seed).random((B * N, in_dim)).astype(np.float32))
    o64 = copy.deepcopy(oracle).double().eval()
    o32 = oracle.eval()
    with torch.no_grad():
        ys = [y.cpu().numpy().reshape(B, N).astype(np.float64) for y in forward_both(model, x.cuda(), B, n)]
        G = graph(n) if graph else mo.line_graph_networkx(n)
        for b in range(B):
            xb = x[b * N:(b + 1) * N]
            ref = o64(G, xb.double()).numpy().reshape(-1)
            own = np.abs(o32(G, xb).double().numpy().reshape(-1) - ref).max() if n < 20 else 0.0
            for y in ys:
                assert np.isfinite(y[b]).all()
                err = np.abs(y[b] - ref)
                # (graphs below 20 nodes: or no further from the exact value than 3x a plain fp32 evaluation, as in
                # test_model_gpu.test_forward_batch_vs_oracle)
                assert (err <= regret_bound(ref)).all() or err.max() <= 3.0 * own, \
                    (model.n_heads, n, b, err.max(), RTOL * np.abs(ref).max(), own)


@pytest.mark.parametrize("H", HEADS)
@pytest.mark.parametrize("n,B,in_dim", [(3, 3, 1), (5, 2, 2), (20, 2, 1), (20, 1, 2), (100, 1, 1)])
def test_forward_vs_oracle(H, n, B, in_dim):
    model, oracle, _ = make_models(H, in_dim)
    check_forward(model, oracle, n, B, in_dim, seed=10 * n + H)


@pytest.mark.parametrize("H", [2])
def test_forward_n200_vs_oracle(H):
    from oracle import model_oracle as mo
    model, oracle, _ = make_models(H)
    check_forward(model, oracle, 200, 1, 1, seed=200, graph=mo.line_graph_arcs_closed_form)


@pytest.mark.parametrize("H", HEADS)
def test_forward_trained_like_weights(H):
    """Trained-like weight scales (oracle.model_oracle.trained_like_state_dict): ill-conditioned in fp32, so the HIP forward
    is held to 3x a plain fp32 evaluation's own distance from the fp64 value (test_model_gpu.test_forward_error_fixtures)."""
    from oracle import model_oracle as mo
    model, oracle, _ = make_models(H, trained_like=True, sd_seed=31)
    model.eval()
    n, B = 30, 2
    N = n * (n - 1) // 2
    x = torch.from_numpy(np.random.default_rng(H).random((B * N, 1)).astype(np.float32))
    G = mo.line_graph_networkx(n)
    o64 = copy.deepcopy(oracle).double().eval()
    with torch.no_grad():
        ys = [y.cpu().numpy().reshape(B, N).astype(np.float64) for y in forward_both(model, x.cuda(), B, n)]
        for b in range(B):
            xb = x[b * N:(b + 1) * N]
            ref = o64(G, xb.double()).numpy().reshape(-1)
            own = np.abs(oracle.eval()(G, xb).double().numpy().reshape(-1) - ref).max()
            for y in ys:
                err = np.abs(y[b] - ref)
                assert (err <= regret_bound(ref)).all() or err.max() <= 3.0 * own, (H, b, err.max(), own)


@pytest.mark.parametrize("H", HEADS)
@pytest.mark.parametrize("scale", [8.0, 300.0])
def test_forward_with_saturated_attention(H, scale):
    """Large attention logits (one dominant source per destination): the factorised weights must not overflow, and beyond a
    logit gap of 60 the direct evaluation is taken."""
    from gnngls_amd.models import EdgePropertyPredictionModel
    from oracle import model_oracle as mo
    _, oracle, sd = make_models(H)
    sd = dict(sd)
    for layer in {0, H - 1}:
        key = f"message_passing_layers.{layer}.message_passing.module.attn_l"
        sd[key] = sd[key] * scale
    oracle.load_state_dict(sd)
    model = EdgePropertyPredictionModel(1, 128, 1, 3, n_heads=H)
    model.load_state_dict(sd)
    model.eval().to("cuda")
    n = 23
    G = mo.line_graph_networkx(n)
    x = torch.rand(G.number_of_nodes(), 1)
    o64 = copy.deepcopy(oracle).double().eval()
    with torch.no_grad():
        ys = forward_both(model, x.cuda(), 1, n)
        ref64 = o64(G, x.double()).numpy().reshape(-1)
        own = np.abs(oracle.eval()(G, x).double().numpy().reshape(-1) - ref64).max()
    for y in ys:
        y = y.cpu().double().numpy().reshape(-1)
        assert np.isfinite(y).all()
        err = np.abs(y - ref64)
        assert (err <= regret_bound(ref64)).all() or err.max() <= 3.0 * own, (H, scale, err.max(), own)


@pytest.mark.parametrize("H", HEADS)
def test_forward_workspace_chunks_are_bitwise_equal(H):
    from gnngls_amd import models as M
    model, _, _ = make_models(H)
    model.eval()
    n, B = 20, 5
    x = torch.rand(B * (n * (n - 1) // 2), 1, device="cuda")
    y_full = M.regret_forward(model, x, B, n)
    model._workspace = None
    y_chunk = M.regret_forward(model, x, B, n, max_workspace_bytes=1)
    assert torch.equal(y_full, y_chunk)


def test_eight_heads_entries_equal_the_old_entries():
    """n_heads = 8 through the *_heads entries is bit for bit the entry without the suffix: forward, prepared forward and the
    training forward + backward."""
    import ctypes
    from gnngls_amd import _lib
    L = _lib.load()
    model, _, _ = make_models(8)
    model.eval()
    n, B, nl = 20, 3, 8
    N = n * (n - 1) // 2
    x = torch.rand(B * N, 1, device="cuda")
    packed = model.pack_weights("cuda")
    ws = torch.empty(int(L.gnngls_regret_forward_workspace_bytes(B, n)), dtype=torch.uint8, device="cuda")
    assert L.gnngls_regret_forward_workspace_bytes_heads(B, n, 8) == ws.numel()
    s = _lib.current_stream()
    ya, yb = torch.empty((B, N), device="cuda"), torch.empty((B, N), device="cuda")
    _lib.check(L.gnngls_regret_forward(_lib.ptr(x), _lib.ptr(packed), B, n, 1, nl, _lib.ptr(ya), _lib.ptr(ws),
                                       ctypes.c_int64(ws.numel()), s))
    _lib.check(L.gnngls_regret_forward_heads(_lib.ptr(x), _lib.ptr(packed), B, n, 1, nl, 8, _lib.ptr(yb), _lib.ptr(ws),
                                             ctypes.c_int64(ws.numel()), s))
    assert torch.equal(ya, yb)
    pa = torch.empty(int(L.gnngls_regret_prepared_bytes(nl)), dtype=torch.uint8, device="cuda")
    pb = torch.empty_like(pa)
    _lib.check(L.gnngls_regret_prepare(_lib.ptr(packed), 1, nl, _lib.ptr(pa), ctypes.c_int64(pa.numel()), s))
    _lib.check(L.gnngls_regret_prepare_heads(_lib.ptr(packed), 1, nl, 8, _lib.ptr(pb), ctypes.c_int64(pb.numel()), s))
    _lib.check(L.gnngls_regret_forward_prepared(_lib.ptr(x), _lib.ptr(packed), _lib.ptr(pa), ctypes.c_int64(pa.numel()), B, n, 1, nl,
                                                _lib.ptr(ya), _lib.ptr(ws), ctypes.c_int64(ws.numel()), s))
    _lib.check(L.gnngls_regret_forward_prepared_heads(_lib.ptr(x), _lib.ptr(packed), _lib.ptr(pb), ctypes.c_int64(pb.numel()), B, n,
                                                      1, nl, 8, _lib.ptr(yb), _lib.ptr(ws), ctypes.c_int64(ws.numel()), s))
    assert torch.equal(ya, yb)
    # training step: the raw image of the module's parameters
    model.train()
    image = torch.cat([p.detach().reshape(-1).float() for p in model.train_parameters()] + [torch.zeros(3, device="cuda")])
    tw = int(L.gnngls_regret_train_workspace_bytes(B, n, nl))
    assert L.gnngls_regret_train_workspace_bytes_heads(B, n, nl, 8) == tw
    out = []
    for heads in (False, True):
        wsp = torch.empty(tw, dtype=torch.uint8, device="cuda")
        y = torch.empty((B * N, 1), device="cuda")
        stats = torch.empty((nl, 2, 2, 128), device="cuda")
        dy = torch.linspace(-1, 1, B * N, device="cuda").reshape(-1, 1)
        g = torch.empty_like(image)
        if heads:
            _lib.check(L.gnngls_regret_train_forward_heads(_lib.ptr(x), _lib.ptr(image), B, n, 1, nl, 8, 1e-5, _lib.ptr(y),
                                                           _lib.ptr(stats), _lib.ptr(wsp), ctypes.c_int64(tw), s))
            _lib.check(L.gnngls_regret_train_backward_heads(_lib.ptr(x), _lib.ptr(image), _lib.ptr(dy), B, n, 1, nl, 8, _lib.ptr(g),
                                                            _lib.ptr(wsp), ctypes.c_int64(tw), s))
        else:
            _lib.check(L.gnngls_regret_train_forward(_lib.ptr(x), _lib.ptr(image), B, n, 1, nl, 1e-5, _lib.ptr(y), _lib.ptr(stats),
                                                     _lib.ptr(wsp), ctypes.c_int64(tw), s))
            _lib.check(L.gnngls_regret_train_backward(_lib.ptr(x), _lib.ptr(image), _lib.ptr(dy), B, n, 1, nl, _lib.ptr(g),
                                                      _lib.ptr(wsp), ctypes.c_int64(tw), s))
        out.append((y, stats, g))
    for a, b in zip(*out):
        assert torch.equal(a, b)


def hip_step(model, n, B, x, target, criterion=None):
    from gnngls_amd.models import LineGraph
    criterion = criterion or torch.nn.MSELoss()
    model.train()
    model.zero_grad()
    y = model(LineGraph(n, batch=B).to("cuda"), x.cuda())
    loss = criterion(y, target.cuda().type_as(y))
    loss.backward()
    torch.cuda.synchronize()
    grads = {k: p.grad.detach().cpu() for k, p in model.named_parameters()}
    return y.detach().cpu(), loss.item(), grads


def check_train_step(H, n, B, bce=False, gat_bias=False):
    from oracle import model_oracle as mo
    model, oracle, _ = make_models(H, seed=4321, sd_seed=77, gat_bias=gat_bias)
    o64 = copy.deepcopy(oracle).double()
    N = n * (n - 1) // 2
    rng = np.random.default_rng(100 * n + H)
    x = torch.from_numpy(rng.random((B * N, 1)).astype(np.float32))
    if bce:
        target = torch.from_numpy((rng.random((B * N, 1)) < 0.2).astype(np.float32))
        pw = len(target) / target.sum() - 1
        c64, c32, c = (torch.nn.BCEWithLogitsLoss(pos_weight=pw.double()), torch.nn.BCEWithLogitsLoss(pos_weight=pw),
                       torch.nn.BCEWithLogitsLoss(pos_weight=pw.cuda()))
    else:
        target = torch.from_numpy(rng.random((B * N, 1)).astype(np.float32))
        c64 = c32 = c = None
    G = mo.batch_line_graphs(n, B) if n < 200 else mo.line_graph_arcs_closed_form(n)
    y32, loss32, g32, _ = mo.train_step_reference(oracle, G, x, target, c32)
    y64, loss64, g64, _ = mo.train_step_reference(o64, G, x.double(), target.double(), c64)
    y, loss, grads = hip_step(model, n, B, x, target, c)
    err = np.abs(y.double().numpy() - y64.numpy()).reshape(-1)
    ref = np.abs(y64.numpy()).reshape(-1)
    own = np.abs(y32.double().numpy() - y64.numpy()).reshape(-1).max()
    assert (err <= 1e-5 * ref + 1e-5 * ref.max() + 3 * own).all(), (H, n, err.max(), own)
    assert abs(loss - loss64.item()) <= 1e-5 * loss64.item() + 3 * abs(loss32.item() - loss64.item())
    m = gradient_error_metrics(grads, g32, g64)
    assert gradient_errors_acceptable(m), (H, n, m)
    return model, grads


@pytest.mark.parametrize("H", HEADS)
@pytest.mark.parametrize("n,B", [(5, 3), (8, 2), (20, 2)])
def test_train_step_vs_oracle(H, n, B):
    check_train_step(H, n, B)


@pytest.mark.parametrize("H,n", [(4, 100), (1, 257)])
def test_train_step_large_vs_oracle(H, n):
    check_train_step(H, n, 1)


@pytest.mark.parametrize("H", HEADS)
def test_train_step_bce_target(H):
    check_train_step(H, 9, 2, bce=True)


@pytest.mark.parametrize("H", [4, 16])
def test_train_step_with_gatconv_bias(H):
    model, grads = check_train_step(H, 10, 2, gat_bias=True)
    keys = [k for k in grads if k.endswith("message_passing.module.bias")]
    assert len(keys) == H and all(grads[k].abs().max().item() == 0.0 for k in keys)


@pytest.mark.parametrize("H", HEADS)
def test_train_rejects_n258(H):
    from gnngls_amd import _lib
    from gnngls_amd.models import LineGraph
    model, _, _ = make_models(H)
    model.train()
    n = 258
    x = torch.zeros((n * (n - 1) // 2, 1), device="cuda")
    with pytest.raises(_lib.GnnglsHipError, match="n=258"):
        model(LineGraph(n).to("cuda"), x)


def test_torch_op_matches_models_forward():
    import gnngls_amd.torch_ops  # noqa: F401
    from gnngls_amd import models as M
    model, _, _ = make_models(4)
    model.eval()
    n, B = 12, 2
    x = torch.rand(B, n * (n - 1) // 2, device="cuda")
    y_op = torch.ops.gnngls.regret_forward(x, model.pack_weights("cuda"), n, 4, 32, 512, 4)
    model.invalidate()
    import ctypes
    from gnngls_amd import _lib
    L = _lib.load()
    packed = model.pack_weights("cuda")
    ws = torch.empty(int(L.gnngls_regret_forward_workspace_bytes_heads(B, n, 4)), dtype=torch.uint8, device="cuda")
    y = torch.empty_like(y_op)
    _lib.check(L.gnngls_regret_forward_heads(_lib.ptr(x), _lib.ptr(packed), B, n, 1, 4, 4, _lib.ptr(y), _lib.ptr(ws),
                                             ctypes.c_int64(ws.numel()), _lib.current_stream()))
    assert torch.equal(y_op, y)
    y_m = M.regret_forward(model, x.reshape(-1, 1), B, n)
    assert torch.allclose(y_op, y_m, rtol=1e-5, atol=1e-5 * y_m.abs().max().item())
    with pytest.raises(NotImplementedError):
        torch.ops.gnngls.regret_forward(x, packed, n, 3, 42, 512, 3)


def test_train_cli_n_heads_4_end_to_end(tmp_path):
    """scripts/train.py --n_heads 4 on a tiny dataset: params.json records n_heads 4, the loss falls, the checkpoints load, and
    scripts/test.py evaluates the best checkpoint with the regret_pred guide."""
    import itertools
    import json
    import pickle
    import subprocess
    import sys

    import networkx as nx
    from sklearn.preprocessing import MinMaxScaler

    from gnngls_amd import datasets
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rng = np.random.default_rng(3)
    data = tmp_path / "tsp10"
    data.mkdir()
    scalers = {"features": MinMaxScaler(), "regret": MinMaxScaler()}
    names = []
    for k in range(12):
        pos = rng.random((10, 2))
        G = nx.Graph()
        for v, p in enumerate(pos):
            G.add_node(v, pos=p)
        for i, j in itertools.combinations(G.nodes, 2):
            w = np.linalg.norm(pos[j] - pos[i])
            G.add_edge(i, j, weight=w, in_solution=False, regret=float(w * w))
        for v in range(10):
            G.edges[v, (v + 1) % 10]["in_solution"] = True
        datasets.set_features(G)
        for key in scalers:
            scalers[key].partial_fit(np.vstack([G.edges[e][key] for e in G.edges]))
        pickle.dump(G, open(data / f"i{k}.pkl", "wb"))
        names.append(f"i{k}.pkl")
    (data / "train.txt").write_text("\n".join(names[:8]) + "\n")
    (data / "val.txt").write_text("\n".join(names[8:]) + "\n")
    (data / "test.txt").write_text("\n".join(names[8:10]) + "\n")
    pickle.dump(scalers, open(data / "scalers.pkl", "wb"))
    tb = tmp_path / "tb"
    subprocess.check_call([sys.executable, os.path.join(root, "scripts", "train.py"), str(data), str(tb), "--batch_size", "4",
                           "--n_epochs", "6", "--checkpoint_freq", "2", "--n_heads", "4", "--use_gpu", "--num_workers", "0"],
                          cwd=root, timeout=600)
    runs = list(tb.iterdir())
    assert len(runs) == 1
    params = json.load(open(runs[0] / "params.json"))
    assert params["n_heads"] == 4 and params["embed_dim"] == 128
    ck = torch.load(runs[0] / "checkpoint_final.pt", map_location="cpu")
    assert ck["model_state_dict"]["message_passing_layers.0.message_passing.module.attn_l"].shape == (1, 4, 32)
    assert "message_passing_layers.3.feed_forward.0.weight" in ck["model_state_dict"]
    assert "message_passing_layers.4.feed_forward.0.weight" not in ck["model_state_dict"]
    scal = [json.loads(line) for line in open(runs[0] / "scalars.jsonl")]
    train_loss = [r["value"] for r in scal if r["tag"] == "Loss/train"]
    assert len(train_loss) == 6 and train_loss[-1] < 0.5 * train_loss[0]
    out = tmp_path / "runs"
    subprocess.check_call([sys.executable, os.path.join(root, "scripts", "test.py"), str(data / "test.txt"),
                           str(runs[0] / "checkpoint_best_val.pt"), str(out), "regret_pred", "--use_gpu", "--time_limit", "0.2"],
                          cwd=root, timeout=600)
    assert any(out.rglob("*"))
