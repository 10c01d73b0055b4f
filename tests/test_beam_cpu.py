"""CPU checks of beam-search decoding (gnngls_beam_search; include/gnngls_hip.h states the definition, gnngls_amd.host.beam_search
restates it).

* Exhaustive widths: width = (n-1)! finds the brute-force minimum of the left-to-right summed score; n = 3 has two leaves.
* width = 1 on integer-valued scores is the greedy nearest-neighbour tour, from any depot.
* The tie rule by hand (constant S, n = 5, width = 3); signed zeros tie.
* Invariants of every result: valid tours, the order of the ranks, select = cost, costs bit for bit.
* Refusal of one instance; the C boundary without a GPU; the Python surfaces.
"""
import ctypes
import inspect
import itertools
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gnngls_amd import host  # noqa: E402


def bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.uint64)


def euclid(rng, n):
    pos = rng.random((n, 2))
    return np.linalg.norm(pos[:, None] - pos[None], axis=2)


def summed(t, M):
    c = np.float64(0.0)
    for x, y in zip(t[:-1], t[1:]):
        c = c + M[x, y]
    return c


def greedy(S, depot):
    """The reference's nearest_neighbor on a dense matrix: the lowest id among the smallest entries."""
    n = S.shape[0]
    tour, seen = [depot], {depot}
    while len(tour) < n:
        i = tour[-1]
        j = min((j for j in range(n) if j not in seen), key=lambda j: (S[i, j], j))
        tour.append(j)
        seen.add(j)
    return tour + [depot]


# ---- exhaustive widths ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4, 5, 6])
def test_exhaustive_width_finds_the_brute_force_minimum(n):
    rng = np.random.default_rng(n)
    for S in (rng.random((n, n)), rng.integers(-3, 4, (n, n)).astype(np.float64), euclid(rng, n)):
        for depot in (0, n - 1):
            others = [j for j in range(n) if j != depot]
            brute = min(summed((depot,) + p + (depot,), S) for p in itertools.permutations(others))
            r = host.beam_search(S, math.factorial(n - 1), depot=depot)
            assert r.status == 0 and r.n_beams == math.factorial(n - 1)
            assert bits(r.best_score) == bits(brute)
            assert bits(summed(r.best_tour, S)) == bits(r.best_score)
            assert len({tuple(t) for t in r.beam_tours.tolist()}) == r.n_beams      # every leaf once


@pytest.mark.parametrize("width", [1, 2, 5])
def test_three_nodes_have_two_leaves(width):
    S = np.array([[9.0, 1.0, 2.0], [3.0, 9.0, 4.0], [5.0, 7.0, 9.0]])
    r = host.beam_search(S, width, D=S)
    assert r.n_beams == min(width, 2) and r.status == 0
    assert r.beam_tours[0].tolist() == [0, 1, 2, 0]                                # 1 + 4 + 5 = 10 against 2 + 7 + 3 = 12: rank by
    assert r.beam_score[0] == 10.0                                                 # the score BEFORE the close, 5 against 9
    if width >= 2:
        assert r.beam_tours[1].tolist() == [0, 2, 1, 0] and r.beam_score[1] == 12.0
    assert (r.beam_tours[r.n_beams:] == -1).all() and np.isnan(r.beam_score[r.n_beams:]).all() and np.isnan(r.beam_cost[r.n_beams:]).all()


# ---- width 1 is the greedy decode ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [5, 64, 100])
def test_width_one_is_nearest_neighbor_on_integer_scores(n):
    rng = np.random.default_rng(100 + n)
    S = rng.integers(0, 6, (n, n)).astype(np.float64)                              # heavy ties, exact partial sums
    for depot in (0, n // 2, n - 1):
        r = host.beam_search(S, 1, depot=depot)
        assert r.n_beams == 1 and r.best_tour.tolist() == greedy(S, depot)
        assert bits(r.best_score) == bits(summed(r.best_tour, S)) and np.isnan(r.best_cost)


# ---- the tie rule --------------------------------------------------------------------------------------------------------------------
def test_constant_scores_keep_pure_k_j_order():
    # step 1: (0,1) (0,2) (0,3); step 2: beam 0 = [0,1] gives j = 2, 3, 4 before any other beam is asked; step 3: beam 0 =
    # [0,1,2] gives 3, 4, then beam 1 = [0,1,3] gives 2; step 4: one candidate per beam
    r = host.beam_search(np.full((5, 5), 2.5), 3, D=np.full((5, 5), 1.0), select="cost")
    assert r.beam_tours.tolist() == [[0, 1, 2, 3, 4, 0], [0, 1, 2, 4, 3, 0], [0, 1, 3, 2, 4, 0]]
    assert r.beam_score.tolist() == [12.5] * 3 and r.beam_cost.tolist() == [5.0] * 3
    assert r.best_tour.tolist() == [0, 1, 2, 3, 4, 0] and r.n_beams == 3
    r = host.beam_search(np.full((5, 5), 2.5), 3, depot=2)
    assert r.beam_tours.tolist() == [[2, 0, 1, 3, 4, 2], [2, 0, 1, 4, 3, 2], [2, 0, 3, 1, 4, 2]]


def test_signed_zeros_tie():
    rng = np.random.default_rng(5)
    for n, width in ((5, 3), (9, 16), (66, 7)):
        Z = np.zeros((n, n))
        M = np.where(rng.random((n, n)) < 0.5, -0.0, 0.0)
        assert np.signbit(M).any() and not np.signbit(M).all()
        a, m = host.beam_search(Z, width, D=Z, select="cost"), host.beam_search(M, width, D=Z, select="cost")
        assert np.array_equal(a.beam_tours, m.beam_tours) and np.array_equal(bits(a.beam_score), bits(m.beam_score))
        assert bits(m.best_score) == bits(0.0)
        # ... and inside sums: 1 + -1 + -0.0 against 1 + -1 + 0.0
        P = rng.integers(-1, 2, (n, n)).astype(np.float64)
        Q = np.where((P == 0) & (rng.random((n, n)) < 0.5), -0.0, P)
        a, m = host.beam_search(P, width), host.beam_search(Q, width)
        assert np.array_equal(a.beam_tours, m.beam_tours) and np.array_equal(bits(a.beam_score), bits(m.beam_score))


# ---- invariants --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,width,depot", [(7, 4, 0), (20, 64, 19), (65, 33, 64), (100, 16, 3)])
def test_invariants_of_one_decode(n, width, depot):
    rng = np.random.default_rng(7 * n + width)
    D = euclid(rng, n)
    for S in (D, rng.random((n, n)) - 0.5, rng.integers(0, 3, (n, n)).astype(np.float64)):
        r = host.beam_search(S, width, depot=depot, D=D, select="cost")
        s = host.beam_search(S, width, depot=depot, D=D, select="score")
        nb = r.n_beams
        assert nb == width and r.status == 0
        pre_close = []
        for k in range(nb):
            t = r.beam_tours[k].tolist()
            assert t[0] == t[-1] == depot and sorted(t[:-1]) == list(range(n))
            assert bits(r.beam_cost[k]) == bits(summed(t, D))
            pre = summed(t[:-1], S)
            pre_close.append(pre if pre != 0 else 0.0)
            tail = pre + S[t[-2], depot]
            assert bits(r.beam_score[k]) == bits(tail if tail != 0 else 0.0)
        assert all(a <= b for a, b in zip(pre_close[:-1], pre_close[1:]))          # ranks ascend in the score before the close
        best = min(range(nb), key=lambda k: (r.beam_cost[k], k))
        assert r.best_tour.tolist() == r.beam_tours[best].tolist() and bits(r.best_cost) == bits(r.beam_cost[best])
        assert bits(r.best_score) == bits(r.beam_score[best])
        best = min(range(nb), key=lambda k: (s.beam_score[k], k))
        assert s.best_tour.tolist() == s.beam_tours[best].tolist() and bits(s.best_score) == bits(s.beam_score[best])
        assert np.array_equal(r.beam_tours, s.beam_tours)                          # select changes the choice only


def test_refusal_is_per_instance_and_ignores_the_diagonal():
    rng = np.random.default_rng(11)
    good = rng.random((6, 6))
    diag = good.copy()
    diag[np.diag_indices(6)] = np.nan
    for bad_value in (np.nan, np.inf, -np.inf):
        bad = good.copy()
        bad[4, 2] = bad_value
        r = [host.beam_search(S, 8, D=good) for S in (good, bad, diag)]
        assert [x.status for x in r] == [0, host.BEAM_STATUS_BAD_SCORE, 0] and host.BEAM_STATUS_BAD_SCORE == 1
        assert r[1].n_beams == 0 and (r[1].best_tour == -1).all() and (r[1].beam_tours == -1).all()
        assert np.isnan(r[1].best_score) and np.isnan(r[1].best_cost) and np.isnan(r[1].beam_score).all() and np.isnan(r[1].beam_cost).all()
        assert np.array_equal(r[0].beam_tours, r[2].beam_tours) and np.array_equal(bits(r[0].beam_score), bits(r[2].beam_score))


def test_range_is_asserted():
    S = np.ones((4, 4))
    for kw in (dict(width=0), dict(width=1025), dict(width=2, depot=4), dict(width=2, depot=-1), dict(width=2, select="cost")):
        with pytest.raises(AssertionError):
            host.beam_search(S, **kw)
    with pytest.raises(AssertionError):
        host.beam_search(np.ones((2, 2)), 1)


# ---- the C ABI without a GPU -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from gnngls_amd import _lib, build
    build.build()
    return _lib.load()


def test_entries_declared_and_exported(lib):
    from gnngls_amd import _lib
    raw = ctypes.CDLL(_lib.SO)
    for name in ("gnngls_beam_search", "gnngls_beam_search_workspace_bytes"):
        assert hasattr(raw, name) and name in _lib.SIGNATURES and name in _lib._BEAM
    args = lib.gnngls_beam_search.argtypes
    assert len(args) == 18 and args[16] is ctypes.c_int64 and lib.gnngls_beam_search_workspace_bytes.restype is ctypes.c_int64
    assert lib.gnngls_abi_version() == 4
    header = open(os.path.join(ROOT, "include", "gnngls_hip.h")).read()
    for word in ("int gnngls_beam_search(", "int64_t gnngls_beam_search_workspace_bytes(int B, int n, int width)", "GNNGLS_BEAM_MAX_N 1024",
                 "GNNGLS_BEAM_MAX_WIDTH 1024", "GNNGLS_BEAM_BAD_SCORE 1", "(key, k, j)"):
        assert word in header, word


def test_workspace_bytes(lib):
    f = lib.gnngls_beam_search_workspace_bytes
    assert f(1, 2, 4) == 0 and f(1, 1025, 4) == 0 and f(1, 5, 0) == 0 and f(1, 5, 1025) == 0 and f(0, 5, 4) == 0
    one = f(1, 100, 128)
    assert one >= 99 * 128 * 4 and one % 16 == 0 and f(7, 100, 128) == 7 * one     # at least the back-pointers; per instance
    assert f(1, 129, 1024) - f(1, 128, 1024) > 2 * 1024 * 3 * 8                    # beyond LDS the visited bits move into it
    assert f(2048, 1024, 1024) > 2 ** 32                                           # int64, not int


def test_argument_checks_answer_before_any_device_work(lib):
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    big = 1 << 40

    def call(B=1, n=5, width=4, depot=0, select=0, S=p, D=None, bt=p, bs=p, bc=p, nb=p, st=p, t=None, s=None, c=None, ws=p, wsb=big):
        return lib.gnngls_beam_search(S, D, B, n, width, depot, select, bt, bs, bc, nb, st, t, s, c, ws, wsb, None)

    hostile = [
        (dict(B=0), -1, b"B=0"), (dict(n=2), -1, b"n=2"), (dict(n=1025), -3, b"n=1025"), (dict(width=0), -1, b"width=0"),
        (dict(width=1025), -3, b"width=1025"), (dict(depot=5), -1, b"depot=5"), (dict(depot=-1), -1, b"depot=-1"),
        (dict(select=2), -1, b"select=2"), (dict(select=1), -1, b"needs the distances"), (dict(S=None), -1, b"NULL"),
        (dict(bt=None), -1, b"NULL"), (dict(bs=None), -1, b"NULL"), (dict(bc=None), -1, b"NULL"), (dict(nb=None), -1, b"NULL"),
        (dict(st=None), -1, b"NULL"), (dict(t=p), -1, b"together"), (dict(s=p, c=p), -1, b"together"), (dict(ws=None), -1, b"workspace"),
        (dict(wsb=lib.gnngls_beam_search_workspace_bytes(1, 5, 4) - 1), -1, b"too small"),
    ]
    for kw, code, msg in hostile:
        assert call(**kw) == code, kw
        err = lib.gnngls_last_error()
        assert err.startswith(b"beam_search:") and msg in err, (kw, err)


def test_python_surface_without_gpu():
    import torch

    from gnngls_amd import _lib, algorithms, ops
    assert str(inspect.signature(ops.beam_search)) == "(S, width, depot=0, D=None, select='score', want_beams=False, workspace=None)"
    assert str(inspect.signature(ops.beam_search_launch)) == str(inspect.signature(ops.beam_search))
    assert (str(inspect.signature(algorithms.beam_search)) ==
            "(G, depot, width, guide='regret_pred', weight='weight', select='cost')")
    assert ops.BEAM_MAX_N == host.BEAM_MAX_N == 1024 and ops.BEAM_MAX_WIDTH == host.BEAM_MAX_WIDTH == 1024
    assert ops.BEAM_BAD_SCORE == host.BEAM_STATUS_BAD_SCORE == 1
    assert [f.name for f in ops.BeamResult.__dataclass_fields__.values()] == [
        "best_tour", "best_score", "best_cost", "n_beams", "status", "beam_tours", "beam_score", "beam_cost"]
    if not torch.cuda.is_available():
        S = torch.ones((1, 4, 4), dtype=torch.float64)
        with pytest.raises(_lib.GnnglsHipError):
            ops.beam_search(S, 2)


def test_torch_op_has_a_shape_function():
    import torch

    import gnngls_amd.torch_ops  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        S = torch.empty((3, 7, 7), dtype=torch.float64, device="cuda")
        for D in (None, S):
            out = torch.ops.gnngls.beam_search(S, D, 5, 0, "score")
            assert [tuple(o.shape) for o in out] == [(3, 8), (3,), (3,), (3,), (3,), (3, 5, 8), (3, 5), (3, 5)]
            assert [o.dtype for o in out] == [torch.int32, torch.float64, torch.float64, torch.int32, torch.int32, torch.int32,
                                              torch.float64, torch.float64]
    with pytest.raises((NotImplementedError, RuntimeError)):                   # HIP key only: no CPU kernel behind the op
        z = torch.zeros((1, 4, 4), dtype=torch.float64)
        torch.ops.gnngls.beam_search(z, None, 2, 0, "score")
