"""CPU checks of alpha-nearness (gnngls_alpha_nearness; the definition in include/gnngls_hip.h): the NumPy restatement
gnngls_amd.host.alpha_nearness -- the reference of the GPU tests -- equals a tree-free brute-force closure bit for bit, and the
boundary is in place: the entry is exported with a ctypes signature, argument errors are answered on the host before any HIP
call, the torch operator has a shape function.  The kernel's arithmetic is pinned on the GPU (tests/test_alpha_gpu.py)."""
import ctypes
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from gnngls_amd import host  # noqa: E402
from test_one_tree_cpu import euclid  # noqa: E402

SIZES = (3, 4, 5, 8, 20, 65, 100, 200)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def closure(D, pi):
    """The definition without any tree: beta = the minimax-path closure of w over nodes 1..n-1 (Floyd-Warshall on (min, max)),
    row 0 from a sort."""
    n = D.shape[0]
    idx = np.arange(n)
    w = ((D + pi[np.minimum.outer(idx, idx)]) + pi[np.maximum.outer(idx, idx)]) + 0.0
    B = w[1:, 1:].copy()
    np.fill_diagonal(B, -np.inf)
    for k in range(n - 1):
        B = np.minimum(B, np.maximum(B[:, k, None], B[None, k, :]))
    alpha = np.zeros((n, n))
    alpha[1:, 1:] = w[1:, 1:] - B
    a0 = w[0, 1:] - np.sort(w[0, 1:])[1]
    alpha[0, 1:] = alpha[1:, 0] = np.where(a0 > 0, a0, 0.0)
    alpha[idx, idx] = 0.0
    return alpha


def tie_heavy(rng, n, levels=4):
    """A symmetric matrix rounded to few distinct values: most comparisons inside Prim are ties."""
    D = np.ceil(euclid(rng, n) * levels)
    np.fill_diagonal(D, 0.0)
    return D


def cases(n):
    rng = np.random.default_rng(1000 + n)
    E = euclid(rng, n)
    T = tie_heavy(rng, n)
    yield "euclid pi=0", E, np.zeros(n), True
    yield "euclid random pi", E, rng.normal(scale=0.1, size=n), True
    yield "ties pi=0", T, np.zeros(n), False
    yield "ties integer pi", T, rng.integers(-2, 3, size=n).astype(float), False


@pytest.mark.parametrize("n", SIZES)
def test_host_reference_equals_the_tree_free_closure(n):
    for what, D, pi, tie_free in cases(n):
        a = host.alpha_nearness(D, pi)
        want = closure(D, pi)
        assert np.array_equal(bits(a), bits(want)), (n, what, np.abs(a - want).max())
        assert np.array_equal(bits(a), bits(a.T)), (n, what)
        assert (a >= 0).all() and not np.signbit(a).any(), (n, what)
        assert (bits(np.diag(a)) == 0).all(), (n, what)
        if tie_free:
            zeros = int((a[np.triu_indices(n, 1)] == 0).sum())
            assert zeros == n, (n, what, zeros)                    # the edges of the minimum 1-tree
    E = euclid(np.random.default_rng(1000 + n), n)
    assert np.array_equal(bits(host.alpha_nearness(E)), bits(host.alpha_nearness(E, np.zeros(n))))


def test_alpha_is_the_cost_of_forcing_an_edge_into_the_one_tree():
    """The definition against its meaning, on an instance small enough to enumerate: minimum 1-tree forced through e minus the
    minimum 1-tree (node 0 joined by its two cheapest edges to a spanning tree of the rest), up to rounding."""
    import itertools
    import networkx as nx
    n = 7
    rng = np.random.default_rng(7)
    D, pi = euclid(rng, n), rng.normal(scale=0.05, size=n)
    w = D + pi[:, None] + pi[None, :]

    def one_tree(forced=None):
        G = nx.Graph()
        for i, j in itertools.combinations(range(1, n), 2):
            G.add_edge(i, j, weight=-1e6 if forced in ((i, j), (j, i)) else w[i, j])
        total = sum(w[i, j] for i, j in nx.minimum_spanning_edges(G, data=False))
        e0 = sorted(range(1, n), key=lambda j: w[0, j])
        pick = e0[:2]
        if forced is not None and 0 in forced:
            j = forced[0] + forced[1]
            pick = [j] + [x for x in e0 if x != j][:1]
        return total + w[0, pick[0]] + w[0, pick[1]]

    base = one_tree()
    a = host.alpha_nearness(D, pi)
    for i, j in itertools.combinations(range(n), 2):
        assert abs(a[i, j] - (one_tree((i, j)) - base)) < 1e-12, (i, j)


@pytest.fixture(scope="module")
def lib():
    from gnngls_amd import _lib, build
    build.build()
    return _lib.load()


def test_entry_exported_with_signature(lib):
    from gnngls_amd import _lib
    raw = ctypes.CDLL(_lib.SO)
    assert hasattr(raw, "gnngls_alpha_nearness") and "gnngls_alpha_nearness" in _lib.SIGNATURES
    assert len(lib.gnngls_alpha_nearness.argtypes) == 7
    assert lib.gnngls_abi_version() == 4
    h = open(os.path.join(ROOT, "include", "gnngls_hip.h")).read()
    for word in ("gnngls_alpha_nearness(", "GNNGLS_ALPHA_MAX_N 1024", "pi[min(i,j)]", "second smallest"):
        assert word in h, word


def test_argument_checks_answer_before_any_device_work(lib):
    """No GPU here: an entry that reached a HIP call would answer GNNGLS_ERR_HIP (-2), not these codes."""
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    hostile = [
        ((None, p, 1, 5, p, p), -1, b"NULL"),
        ((p, p, 1, 5, None, p), -1, b"NULL"),
        ((p, None, 1, 5, p, None), -1, b"NULL"),
        ((p, p, 1, 2, p, p), -1, b"n=2"),
        ((p, p, 1, 1025, p, p), -3, b"n=1025"),
        ((p, p, 0, 5, p, p), -1, b"B=0"),
        ((p, p, -1, 5, p, p), -1, b"B=-1"),
    ]
    for args, code, msg in hostile:
        assert lib.gnngls_alpha_nearness(*args, None) == code, args
        err = lib.gnngls_last_error()
        assert b"alpha_nearness" in err and msg in err, (args, err)


def test_torch_op_has_a_shape_function_and_no_cpu_kernel():
    import torch
    import gnngls_amd.torch_ops as T
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert "Ten operators" in T.__doc__
    with FakeTensorMode():
        D = torch.empty((5, 9, 9), dtype=torch.float64, device="cuda")
        pi = torch.empty((5, 9), dtype=torch.float64, device="cuda")
        for arg in (pi, None):
            a = torch.ops.gnngls.alpha_nearness(D, arg)
            assert a.shape == (5, 9, 9) and a.dtype == torch.float64
    with pytest.raises(NotImplementedError):
        torch.ops.gnngls.alpha_nearness(torch.zeros((1, 4, 4), dtype=torch.float64), None)


def test_python_surface():
    from gnngls_amd import algorithms, ops, pipeline
    sig = inspect.signature(pipeline.solve_batch)
    assert sig.parameters["alpha_iters"].default == sig.parameters["bound_iters"].default == 2000
    assert list(inspect.signature(ops.alpha_nearness).parameters) == ["D", "pi"]
    assert list(inspect.signature(host.alpha_nearness).parameters) == ["D", "pi"]
    sig = inspect.signature(algorithms.alpha_nearness)
    assert list(sig.parameters) == ["G", "weight", "attr", "max_iters"]
    assert (sig.parameters["weight"].default, sig.parameters["attr"].default, sig.parameters["max_iters"].default) == ("weight", "alpha", 2000)
    assert ops.ALPHA_MAX_N == 1024


def test_cli_names_the_flag():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "test.py"), "--help"], capture_output=True, text=True, cwd=ROOT)
    assert out.returncode == 0 and "--alpha_iters" in out.stdout
