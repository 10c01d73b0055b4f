"""Head counts other than 8 without a GPU: which architectures the HIP path accepts, the weight image of a 4-head model, and the
C entry points of include/gnngls_hip.h for n_heads (symbols, answers, and refusal of an unsupported n_heads before any device
work)."""
import ctypes
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "gnngls_amd", "libgnngls_hip.so")
NEW_SYMBOLS = ["gnngls_model_heads_supported", "gnngls_regret_forward_workspace_bytes_heads", "gnngls_regret_forward_heads",
               "gnngls_regret_prepare_heads", "gnngls_regret_forward_prepared_heads", "gnngls_regret_train_workspace_bytes_heads",
               "gnngls_regret_train_forward_heads", "gnngls_regret_train_backward_heads"]
GNNGLS_ERR_UNSUPPORTED = -3


def lib():
    if not os.path.isfile(SO):
        pytest.fail(f"{SO} missing: run __graft_entry__.build() first")
    from gnngls_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("H", [1, 2, 4, 8, 16])
def test_supported_head_counts_are_accepted(H):
    from gnngls_amd.models import EdgePropertyPredictionModel
    m = EdgePropertyPredictionModel(1, 128, 1, 3, n_heads=H)
    m._check_supported()
    assert len(m.message_passing_layers) == H


@pytest.mark.parametrize("H", [3, 32, 64])
def test_other_head_counts_are_rejected(H):
    from gnngls_amd.models import EdgePropertyPredictionModel
    m = EdgePropertyPredictionModel.__new__(EdgePropertyPredictionModel)
    torch.nn.Module.__init__(m)
    m.embed_dim, m.n_heads, m.out_dim = 128, H, 1        # (3 does not divide 128; the constructor itself is the reference's)
    with pytest.raises(NotImplementedError, match=r"\{1, 2, 4, 8, 16\}"):
        m._check_supported()


@pytest.mark.parametrize("embed_dim,H", [(64, 4), (256, 8), (96, 2)])
def test_other_embed_dims_are_rejected(embed_dim, H):
    from gnngls_amd.models import EdgePropertyPredictionModel
    with pytest.raises(NotImplementedError):
        EdgePropertyPredictionModel(1, embed_dim, 1, 3, n_heads=H).pack_weights("cpu")


def test_four_head_weight_image():
    from gnngls_amd.models import EdgePropertyPredictionModel
    L = lib()
    torch.manual_seed(0)
    m = EdgePropertyPredictionModel(2, 128, 1, 3, n_heads=4)
    packed = m.pack_weights("cpu")
    assert packed.numel() == L.gnngls_model_packed_floats(2, 4) == 128 * 2 + 128 + 4 * (
        128 * 128 + 4 * 128 + 512 * 128 + 512 + 128 * 512 + 3 * 128) + 128 + 4
    off = 128 * 2 + 128
    layer = 128 * 128 + 4 * 128 + 512 * 128 + 512 + 128 * 512 + 3 * 128
    for k, lay in enumerate(m.message_passing_layers):
        gat = lay.message_passing.module
        assert gat.attn_l.shape == (1, 4, 32)
        base = off + k * layer + 128 * 128
        assert torch.equal(packed[base:base + 128], gat.attn_l.detach().reshape(-1))          # head-major (h, f)
        assert torch.equal(packed[base + 128:base + 256], gat.attn_r.detach().reshape(-1))
        assert torch.equal(packed[base:base + 32], gat.attn_l.detach()[0, 0])


def test_new_symbols_and_abi_version():
    L = lib()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
    assert L.gnngls_abi_version() == 4
    assert [H for H in range(0, 70) if L.gnngls_model_heads_supported(H)] == [1, 2, 4, 8, 16]
    assert L.gnngls_model_heads_supported(-8) == 0


def test_workspace_queries():
    L = lib()
    for B, n in [(1, 5), (3, 100)]:
        N = n * (n - 1) // 2
        base = L.gnngls_regret_forward_workspace_bytes(B, n)
        for H in (1, 2, 4, 8):
            assert L.gnngls_regret_forward_workspace_bytes_heads(B, n, H) == base
        assert L.gnngls_regret_forward_workspace_bytes_heads(B, n, 16) == base + B * N * 2 * 32 * 4
        tw = L.gnngls_regret_train_workspace_bytes(B, n, 3)
        for H in (1, 2, 4, 8):
            assert L.gnngls_regret_train_workspace_bytes_heads(B, n, 3, H) == tw
        assert L.gnngls_regret_train_workspace_bytes_heads(B, n, 3, 16) > tw
        for H in (0, 3, 32):
            assert L.gnngls_regret_forward_workspace_bytes_heads(B, n, H) == 0
            assert L.gnngls_regret_train_workspace_bytes_heads(B, n, 3, H) == 0


@pytest.mark.parametrize("H", [0, 3, 5, 32, 64])
def test_unsupported_heads_fail_before_device_work(H):
    """Every new entry refuses a bad n_heads with GNNGLS_ERR_UNSUPPORTED -- with NULL device pointers, so nothing can have
    been enqueued -- and names the supported set."""
    L = lib()
    null = None
    one = ctypes.c_int64(1 << 20)
    calls = {
        "gnngls_regret_forward_heads": lambda: L.gnngls_regret_forward_heads(null, null, 1, 10, 1, H, H, null, null, one, null),
        "gnngls_regret_prepare_heads": lambda: L.gnngls_regret_prepare_heads(null, 1, H, H, null, one, null),
        "gnngls_regret_forward_prepared_heads": lambda: L.gnngls_regret_forward_prepared_heads(
            null, null, null, one, 1, 10, 1, H, H, null, null, one, null),
        "gnngls_regret_train_forward_heads": lambda: L.gnngls_regret_train_forward_heads(
            null, null, 1, 10, 1, H, H, 1e-5, null, null, null, one, null),
        "gnngls_regret_train_backward_heads": lambda: L.gnngls_regret_train_backward_heads(
            null, null, null, 1, 10, 1, H, H, null, null, one, null),
    }
    for name, call in calls.items():
        assert call() == GNNGLS_ERR_UNSUPPORTED, name
        assert b"{1, 2, 4, 8, 16}" in L.gnngls_last_error(), name


def test_supported_heads_still_check_their_arguments():
    """A supported n_heads with NULL pointers is an argument error (GNNGLS_ERR_ARG), not an unsupported head count."""
    L = lib()
    one = ctypes.c_int64(1 << 20)
    for H in (1, 16):
        rc = L.gnngls_regret_forward_prepared_heads(None, None, None, one, 1, 10, 1, H, H, None, None, one, None)
        assert rc not in (0, GNNGLS_ERR_UNSUPPORTED)
        rc = L.gnngls_regret_train_forward_heads(None, None, 1, 10, 1, H, H, 1e-5, None, None, None, one, None)
        assert rc not in (0, GNNGLS_ERR_UNSUPPORTED)


def test_torch_op_shape_function_accepts_head_shapes():
    """The fake (meta) registration of gnngls::regret_forward serves every supported (heads, head_dim) shape."""
    pytest.importorskip("torch._subclasses.fake_tensor")
    from torch._subclasses.fake_tensor import FakeTensorMode
    import gnngls_amd.torch_ops  # noqa: F401
    n = 10
    with FakeTensorMode():
        feat = torch.empty(3, n * (n - 1) // 2)
        for H in (1, 2, 4, 8, 16):
            w = torch.empty(1000)
            y = torch.ops.gnngls.regret_forward(feat, w, n, H, 128 // H, 512, H)
            assert tuple(y.shape) == (3, n * (n - 1) // 2)
