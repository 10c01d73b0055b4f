"""CPU checks of the Held-Karp 1-tree bound's boundary (gnngls_one_tree_bound; oracle/one_tree.c on the device): the entry is
exported with a ctypes signature, the header carries its constants, argument errors are answered on the host before any HIP
call, and the Python surfaces carry the new switches.  The arithmetic is pinned on the GPU (tests/test_one_tree_bound_gpu.py)."""
import ctypes
import inspect
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from gnngls_amd import _lib, build
    build.build()
    return _lib.load()


def header():
    return open(os.path.join(ROOT, "include", "gnngls_hip.h")).read()


def test_entry_exported_with_signature(lib):
    from gnngls_amd import _lib
    raw = ctypes.CDLL(_lib.SO)
    assert hasattr(raw, "gnngls_one_tree_bound") and "gnngls_one_tree_bound" in _lib.SIGNATURES
    assert len(lib.gnngls_one_tree_bound.argtypes) == 11
    assert lib.gnngls_abi_version() == 4
    # the launch has a profile kind of its own, behind the kinds that existed (no index moved)
    assert _lib.PROF_KINDS[-1] == "insertion" and _lib.PROF_KINDS_BOUNDS == ["one_tree_bound"]
    enum = re.search(r"enum \{\s*GNNGLS_PROF_PACK = 0,(.*?)\};", header(), flags=re.S).group(1)
    kinds = re.findall(r"GNNGLS_PROF_[A-Z0-9_]+", enum)
    assert kinds[-2:] == ["GNNGLS_PROF_ONE_TREE_BOUND", "GNNGLS_PROF_KINDS"]
    assert len(kinds) == len(_lib.PROF_KINDS) + len(_lib.PROF_KINDS_BOUNDS)      # (GNNGLS_PROF_PACK sits in front of the match)


def test_header_constants():
    h = header()
    for word in ("gnngls_one_tree_bound(", "GNNGLS_ONE_TREE_MAX_N 1024", "GNNGLS_BOUND_EXIT_ITERS 0", "GNNGLS_BOUND_EXIT_STEP 1",
                 "GNNGLS_BOUND_EXIT_TOUR 2", "oracle/one_tree.c", "scripts/test.py:62,104", "GNNGLS_STATUS_ASYMMETRIC"):
        assert word in h, word
    from gnngls_amd import ops
    assert (ops.BOUND_EXIT_ITERS, ops.BOUND_EXIT_STEP, ops.BOUND_EXIT_TOUR) == (0, 1, 2) and ops.ONE_TREE_MAX_N == 1024


def test_argument_checks_answer_before_any_device_work(lib):
    """No GPU here: an entry that reached a HIP call would answer GNNGLS_ERR_HIP (-2), not these codes."""
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    call = lambda D, ub, B, n, iters, bound, pi=p: lib.gnngls_one_tree_bound(D, ub, B, n, iters, bound, pi, p, p, p, None)  # noqa: E731
    hostile = [
        ((p, p, 1, 2, 10, p), -1, b"n=2"),
        ((p, p, 1, 1025, 10, p), -3, b"n=1025"),
        ((p, p, 1, 5, -1, p), -1, b"max_iters=-1"),
        ((None, p, 1, 5, 10, p), -1, b"NULL"),
        ((p, None, 1, 5, 10, p), -1, b"NULL"),
        ((p, p, 1, 5, 10, None), -1, b"NULL"),
        ((p, p, -1, 5, 10, p), -1, b"B=-1"),
    ]
    for args, code, msg in hostile:
        assert call(*args) == code, args
        err = lib.gnngls_last_error()
        assert b"one_tree_bound" in err and msg in err, (args, err)
    assert call(None, None, 0, 5, 10, None, None) == 0            # an empty batch: nothing to launch


def test_launch_query(lib):
    from gnngls_amd import ops
    # one wavefront per instance up to n = 256 with 1..4 nodes per lane, then 2..4 wavefronts of 4 nodes per lane
    for n, threads, slots in ((3, 64, 1), (64, 64, 1), (65, 64, 2), (100, 64, 2), (129, 64, 3), (200, 64, 4), (256, 64, 4),
                              (257, 128, 4), (512, 128, 4), (513, 192, 4), (1024, 256, 4)):
        d = ops.one_tree_describe(n)
        assert (d["threads"], d["nodes_per_lane"]) == (threads, slots), (n, d)
        assert d["threads"] * d["nodes_per_lane"] >= n and n * 8 <= d["lds_bytes"] <= n * 8 + 512
    assert lib.gnngls_one_tree_bound_describe(2, None, None, None) == -1
    assert lib.gnngls_one_tree_bound_describe(1025, None, None, None) == -1


def test_python_surface():
    from gnngls_amd import pipeline
    import gnngls_amd
    sig = inspect.signature(pipeline.solve_batch)
    assert sig.parameters["lower_bound"].default is False and sig.parameters["bound_iters"].default == 2000
    fields = pipeline.SolveResult.__dataclass_fields__
    assert fields["lower_bound"].default is None and fields["bound_exit"].default is None
    sig = inspect.signature(gnngls_amd.lower_bound)
    assert list(sig.parameters) == ["G", "tour", "weight", "max_iters"] and sig.parameters["max_iters"].default == 2000


def test_cli_names_the_flag():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "test.py"), "--help"], capture_output=True, text=True, cwd=ROOT)
    assert out.returncode == 0 and "--lower_bound" in out.stdout


def test_torch_op_has_a_shape_function():
    import torch
    import gnngls_amd.torch_ops  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        D = torch.empty((5, 9, 9), dtype=torch.float64, device="cuda")
        ub = torch.empty((5,), dtype=torch.float64, device="cuda")
        bound, pi, iters, exit_kind, status = torch.ops.gnngls.one_tree_bound(D, ub, 100)
    assert bound.shape == (5,) and bound.dtype == torch.float64 and pi.shape == (5, 9) and pi.dtype == torch.float64
    assert iters.shape == exit_kind.shape == status.shape == (5,) and iters.dtype == torch.int32
