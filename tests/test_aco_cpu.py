"""CPU checks of the MAX-MIN ant system (gnngls_aco_run; include/gnngls_hip.h states the definition, gnngls_amd.host.aco restates it).

* host.sampled_walk is the walk tests/test_sampling_cpu.py restates (invert = 0), from any depot, at the lane and slot edges.
* One update by hand at n = 4: evaporation, deposit, both clamps, the diagonal, symmetry.
* The rules by hand: the gb_every schedule, the lowest-index tie, the strict < for the best pair, the early end.
* Chaining, the Philox stream (counter word 3 = 2), the C boundary without a GPU, the Python surfaces.
* Sanity of the definition: on Euclidean instances the colony ends below its first iteration.
"""
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from test_sampling_cpu import philox_uniforms as walk_uniforms  # noqa: E402
from test_sampling_cpu import restated_walk  # noqa: E402

from gnngls_amd import host  # noqa: E402

BAD_WEIGHTS = 6


def bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.uint64)


def euclid(rng, n):
    pos = rng.random((n, 2))
    return np.linalg.norm(pos[:, None] - pos[None], axis=2)


def inverse_square(D):
    with np.errstate(divide="ignore"):
        return np.where(~np.eye(D.shape[0], dtype=bool), D ** -2.0, 0.0)


def tour_cost(t, D):
    c = np.float64(0.0)
    for x, y in zip(t[:-1], t[1:]):
        c = c + D[x, y]
    return c


# ---- the walk ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [5, 64, 65, 130])
def test_sampled_walk_is_the_restated_walk(n):
    rng = np.random.default_rng(n)
    for depot in (0, n // 2, n - 1):
        W = rng.uniform(0.1, 3.0, size=(n, n))
        u = rng.random(n - 1)
        u[::7] = 0.0
        u[3::7] = np.nextafter(1.0, 0.0)
        assert host.sampled_walk(W, depot, u) == restated_walk(W, depot, False, u)
        W[rng.integers(0, n, 2 * n), rng.integers(0, n, 2 * n)] = 0.0          # zero weights are never picked
        assert host.sampled_walk(W, depot, u) == restated_walk(W, depot, False, u)
        W[depot, :] = 0.0                                                       # the all-zero rule at the first step
        W[(depot + 1) % n, (depot + 2) % n] = np.inf                            # the inf rule wherever that node is left
        assert host.sampled_walk(W, depot, u) == restated_walk(W, depot, False, u)
    for bad in (np.nan, -1.0):
        W = rng.uniform(0.1, 3.0, size=(n, n))
        W[0, 1:] = bad
        assert host.sampled_walk(W, 0, rng.random(n - 1)) is None and restated_walk(W, 0, False, rng.random(n - 1)) is None
    assert host.sampled_walk(np.full((n, n), 1e308), 0, rng.random(n - 1)) is None     # the total overflows


# ---- one update by hand ---------------------------------------------------------------------------------------------------------
SQUARE = np.array([[0.0, 1.0, 2.0, 1.0],
                   [1.0, 0.0, 1.0, 2.0],
                   [2.0, 1.0, 0.0, 1.0],
                   [1.0, 2.0, 1.0, 0.0]])          # the tour 0-1-2-3-0 costs 4, 0-1-3-2-0 and 0-2-1-3-0 cost 6


def test_one_update_by_hand():
    # H makes the single ant (from node 0) walk 0 -> 1 -> 2 -> 3 whatever u is: every other candidate weighs 0
    H = np.zeros((4, 4))
    H[0, 1] = H[1, 2] = H[2, 3] = 1.0
    tau = np.full((4, 4), 0.5)
    tau[0, 2] = tau[2, 0] = 0.02          # evaporates below tau_min
    tau[0, 1] = tau[1, 0] = 2.6           # deposit pushes it over tau_max
    tau[1, 1] = 7.0                       # the diagonal is never written
    r = host.aco(SQUARE, H, ants=1, iters=1, rho=0.1, min_ratio=0.01, spread_starts=False, u=np.full((1, 1, 3), 0.5), tau=tau)
    assert r.status == 0 and r.iters_done == 1 and r.best_tour == [0, 1, 2, 3, 0] and r.best_cost == 4.0 and r.trace == [4.0]
    keep, q, tmax = np.float64(1.0) - np.float64(0.1), np.float64(1.0) / np.float64(4.0), np.float64(1.0) / (np.float64(0.1) * np.float64(4.0))
    tmin = tmax * np.float64(0.01)
    assert tmax == 2.5 and q == 0.25
    want = np.empty((4, 4))
    want[:] = np.float64(0.5) * keep                                          # off the tour: evaporation only
    for i, j in ((1, 2), (2, 3), (3, 0)):
        want[i, j] = want[j, i] = np.float64(0.5) * keep + q                  # on the tour: evaporation, then the deposit
    want[0, 2] = want[2, 0] = tmin                                            # 0.018 < 0.025
    want[0, 1] = want[1, 0] = tmax                                            # 2.34 + 0.25 > 2.5
    want[np.arange(4), np.arange(4)] = (0.5, 7.0, 0.5, 0.5)
    assert np.float64(0.02) * keep < tmin and np.float64(2.6) * keep + q > tmax
    assert np.array_equal(bits(r.tau), bits(want))
    assert np.array_equal(bits(r.tau), bits(r.tau.T))                         # a symmetric tau stays bitwise symmetric
    assert np.array_equal(r.ant_tours, [[0, 1, 2, 3, 0]]) and r.ant_cost.tolist() == [4.0]
    # the start node does not change the cost: the walk from node 2 is 2 -> 3, then (all-zero rule, u = 0) 0, then 1
    r2 = host.aco(SQUARE, H, ants=1, iters=1, rho=0.1, min_ratio=0.01, spread_starts=True, iter0=2, u=np.zeros((1, 1, 3)), tau=tau)
    assert r2.best_tour == [0, 1, 2, 3, 0] and r2.best_cost == 4.0 and np.array_equal(bits(r2.tau), bits(want))


def test_min_ratio_one_pins_every_entry_to_tau_max():
    D = euclid(np.random.default_rng(3), 7)
    r = host.aco(D, inverse_square(D), ants=3, iters=4, rho=0.2, min_ratio=1.0, seed=5)
    tmax = np.float64(1.0) / (np.float64(0.2) * r.best_cost)
    off = ~np.eye(7, dtype=bool)
    assert (bits(r.tau[off]) == bits(tmax)).all() and r.best_cost == min(r.trace)


# ---- the rules by hand ------------------------------------------------------------------------------------------------------------
def test_gb_every_schedule():
    # iteration 0 finds the square's perimeter (cost 4); iteration 1 is forced onto 0-2-1-3-0 (cost 6).  With gb_every = 2 the
    # deposit of iteration 1 (g + 1 = 2) goes to the BEST tour's edges with q = 1 / 4, without it to the ant's with q = 1 / 6.
    H0 = np.zeros((4, 4))
    H0[0, 1] = H0[1, 2] = H0[2, 3] = 1.0
    first = host.aco(SQUARE, H0, ants=1, iters=1, rho=0.5, min_ratio=1e-3, spread_starts=False, u=np.zeros((1, 1, 3)), tau=np.ones((4, 4)))
    H1 = np.zeros((4, 4))
    H1[0, 2] = H1[2, 1] = H1[1, 3] = 1.0
    out = {}
    for gb in (0, 2, 3):
        out[gb] = host.aco(SQUARE, H1, ants=1, iters=1, iter0=1, rho=0.5, min_ratio=1e-3, gb_every=gb, spread_starts=False,
                           u=np.zeros((1, 1, 3)), tau=first.tau, best_tour=first.best_tour, best_cost=first.best_cost)
        assert out[gb].best_tour == [0, 1, 2, 3, 0] and out[gb].best_cost == 4.0 and out[gb].trace == [6.0]
    keep = np.float64(0.5)
    assert out[2].tau[0, 1] == first.tau[0, 1] * keep + np.float64(1.0) / np.float64(4.0)          # a best-tour edge
    assert out[2].tau[0, 2] == first.tau[0, 2] * keep                                               # the ant's edge: nothing
    assert out[0].tau[0, 2] == first.tau[0, 2] * keep + np.float64(1.0) / np.float64(6.0)
    assert out[0].tau[0, 1] == first.tau[0, 1] * keep
    assert np.array_equal(bits(out[3].tau), bits(out[0].tau))                                       # (1 + 1) % 3 != 0


def test_lowest_index_tie_and_strict_less():
    n = 6
    D = np.ones((n, n)) - np.eye(n)                                            # every tour costs n
    rng = np.random.default_rng(0)
    u = rng.random((3, 4, n - 1))
    r = host.aco(D, np.ones((n, n)), ants=4, iters=3, rho=0.1, spread_starts=False, u=u, tau=np.ones((n, n)))
    first = host.aco(D, np.ones((n, n)), ants=4, iters=1, rho=0.1, spread_starts=False, u=u[:1], tau=np.ones((n, n)))
    assert first.best_tour == first.ant_tours[0].tolist()                      # the tie goes to ant 0
    assert len({tuple(t) for t in first.ant_tours.tolist()}) > 1               # ... although the ants differ
    assert r.best_tour == first.best_tour and r.trace == [float(n)] * 3        # an equal cost never replaces the best
    assert r.ant_tours[0].tolist() != r.best_tour                              # ... although iteration 2's winner is another tour
    # the deposit of every iteration went to ant 0's tour of THAT iteration
    t = r.ant_tours[0].tolist()
    assert r.tau[t[0], t[1]] > r.tau.min()


def test_early_end_on_a_nan_row():
    n = 6
    D = euclid(np.random.default_rng(1), n)
    H = inverse_square(D)
    good = host.aco(D, H, ants=3, iters=2, seed=3)
    Hbad = H.copy()
    Hbad[2, :] = np.nan
    r = host.aco(D, Hbad, ants=3, iters=4, seed=3)
    assert r.status == BAD_WEIGHTS and r.iters_done == 0 and r.trace == [] and r.best_tour is None and np.isinf(r.best_cost)
    assert np.array_equal(bits(r.tau), bits(host.aco_init_tau(D, 0.1)))
    # an end in a later iteration keeps what the earlier ones left: feed the good run's state to a run on the bad heuristic
    r = host.aco(D, Hbad, ants=3, iters=3, iter0=2, seed=3, tau=good.tau, best_tour=good.best_tour, best_cost=good.best_cost)
    assert r.status == BAD_WEIGHTS and r.iters_done == 0 and r.best_tour == good.best_tour and r.best_cost == good.best_cost
    assert np.array_equal(bits(r.tau), bits(good.tau))
    # costs that are not finite, or not positive, end the run as well
    Dinf = D.copy()
    Dinf[0, :] = Dinf[:, 0] = np.inf
    assert host.aco(Dinf, H, ants=2, iters=2).status == BAD_WEIGHTS
    assert host.aco(np.zeros((n, n)), np.ones((n, n)), ants=2, iters=2, tau=np.ones((n, n))).status == BAD_WEIGHTS


def test_chaining_is_the_longer_run():
    n = 9
    D = euclid(np.random.default_rng(2), n)
    H = inverse_square(D)
    for gb in (0, 2):
        whole = host.aco(D, H, ants=5, iters=7, gb_every=gb, seed=11, b=3)
        a = host.aco(D, H, ants=5, iters=3, gb_every=gb, seed=11, b=3)
        z = host.aco(D, H, ants=5, iters=4, iter0=3, gb_every=gb, seed=11, b=3, tau=a.tau, best_tour=a.best_tour, best_cost=a.best_cost)
        assert np.array_equal(bits(z.tau), bits(whole.tau)) and z.best_tour == whole.best_tour
        assert bits(z.best_cost) == bits(whole.best_cost) and a.trace + z.trace == whole.trace
        assert np.array_equal(z.ant_tours, whole.ant_tours)


def test_philox_stream_two():
    n, R, K, iter0, seed = 8, 3, 4, 5, 99
    D = euclid(np.random.default_rng(4), n)
    H = inverse_square(D)
    u = host.philox_uniforms(seed, 2, K * R, n - 1, k0=iter0 * R, c3=2).reshape(2, K, R, n - 1)
    for b in range(2):
        x, y = host.aco(D, H, ants=R, iters=K, iter0=iter0, seed=seed, b=b), host.aco(D, H, ants=R, iters=K, iter0=iter0, u=u[b])
        assert np.array_equal(bits(x.tau), bits(y.tau)) and x.best_tour == y.best_tour and x.trace == y.trace
    for c3 in (0, 1):
        assert not np.array_equal(u, host.philox_uniforms(seed, 2, K * R, n - 1, k0=iter0 * R, c3=c3).reshape(u.shape))
    assert np.array_equal(host.philox_uniforms(seed, 2, K * R, n - 1, c3=0), walk_uniforms(seed, 2, K * R, n - 1))
    header = open(os.path.join(ROOT, "include", "gnngls_hip.h")).read()
    philox = open(os.path.join(ROOT, "gnngls_amd", "csrc", "philox.h")).read()
    assert "(b, g * ants + a, step, 2)" in header and "2 = the ants'" in philox


def test_heuristic():
    rng = np.random.default_rng(6)
    G = rng.uniform(0.5, 2.0, size=(2, 5, 5))
    H = host.aco_heuristic(G, 2.0, "inverse")
    off = ~np.eye(5, dtype=bool)
    assert np.allclose(H[:, off], G[:, off] ** -2.0, rtol=1e-15) and (H[:, ~off] == 0).all()
    G = rng.normal(size=(2, 5, 5))                                             # scores that reach below 0
    G[:, ~off] = 1e9                                                           # the diagonal takes no part in min and mean
    S = host.aco_heuristic(G, 2.0, "shifted")
    for b in range(2):
        g = G[b][off]
        assert np.allclose(S[b][off], ((g - g.min()) / (g.mean() - g.min()) + 0.1) ** -2.0, rtol=1e-12)
        assert S[b][off].max() == pytest.approx(100.0) and (S[b][off] > 0).all() and (S[b][~off] == 0).all()
    assert host.aco_heuristic(G[0], 1.0, "shifted").shape == (5, 5)
    with pytest.raises(ValueError, match="kind"):
        host.aco_heuristic(G, 2.0, "other")


# ---- the C ABI without a GPU -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from gnngls_amd import _lib, build
    build.build()
    return _lib.load()


def test_entry_exported_with_signature(lib):
    from gnngls_amd import _lib
    raw = ctypes.CDLL(_lib.SO)
    assert hasattr(raw, "gnngls_aco_run") and "gnngls_aco_run" in _lib.SIGNATURES
    args = lib.gnngls_aco_run.argtypes
    assert len(args) == 22 and args[9] is ctypes.c_int64 and args[14] is ctypes.c_uint64 and args[10] is ctypes.c_double
    assert lib.gnngls_abi_version() == 4
    header = open(os.path.join(ROOT, "include", "gnngls_hip.h")).read()
    for word in ("gnngls_aco_run(", "GNNGLS_ACO_MAX_N 1024", "GNNGLS_ACO_MAX_ANTS 256", "tau_min = tau_max * min_ratio", "Chaining"):
        assert word in header, word


def test_argument_checks_answer_before_any_device_work(lib):
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(B=1, n=5, ants=4, iters=2, iter0=0, rho=0.1, min_ratio=0.1, gb_every=0, D=p, H=p, tau=p, bt=p, bc=p, done=p, st=p, at=None,
             ac=None):
        return lib.gnngls_aco_run(D, H, tau, bt, bc, B, n, ants, iters, iter0, rho, min_ratio, gb_every, 1, 0, None, done, st, None, at,
                                  ac, None)

    hostile = [
        (dict(B=0), -1, b"B=0"), (dict(n=2), -1, b"n=2"), (dict(n=1025), -3, b"n=1025"), (dict(ants=0), -1, b"ants=0"),
        (dict(ants=257), -3, b"ants=257"), (dict(iters=-1), -1, b"iters=-1"), (dict(iter0=-1), -1, b"iter0=-1"),
        (dict(rho=0.0), -1, b"rho=0"), (dict(rho=1.0), -1, b"rho=1"), (dict(rho=float("nan")), -1, b"rho="),
        (dict(min_ratio=0.0), -1, b"min_ratio=0"), (dict(min_ratio=1.5), -1, b"min_ratio=1.5"), (dict(gb_every=-1), -1, b"gb_every=-1"),
        (dict(iter0=2 ** 30 - 1, iters=1, ants=4), -1, b"2^32"), (dict(iter0=2 ** 40), -1, b"2^32"),
        (dict(D=None), -1, b"NULL"), (dict(H=None), -1, b"NULL"), (dict(tau=None), -1, b"NULL"), (dict(bt=None), -1, b"NULL"),
        (dict(bc=None), -1, b"NULL"), (dict(done=None), -1, b"NULL"), (dict(st=None), -1, b"NULL"), (dict(at=p), -1, b"together"),
    ]
    for kw, code, msg in hostile:
        assert call(**kw) == code, kw
        err = lib.gnngls_last_error()
        assert err.startswith(b"aco_run:") and msg in err, (kw, err)


def test_python_surface_without_gpu():
    import torch

    from gnngls_amd import _lib, ops
    assert (str(inspect.signature(ops.aco)) == "(D, H, ants=16, iters=100, rho=0.1, min_ratio=None, gb_every=0, spread_starts=True, seed=0, "
            "u=None, iter0=0, tau=None, best_tour=None, best_cost=None, want_trace=False, want_ants=False)")
    assert list(inspect.signature(ops.aco_heuristic).parameters) == ["G", "beta", "kind"]
    assert list(inspect.signature(ops.aco_init_tau).parameters) == ["D", "rho"]
    assert ops.ACO_MAX_N == host.ACO_MAX_N == 1024 and ops.ACO_MAX_ANTS == host.ACO_MAX_ANTS == 256
    assert host.ACO_STATUS_BAD_WEIGHTS == ops.SAMPLE_BAD_WEIGHTS == BAD_WEIGHTS
    if not torch.cuda.is_available():
        D = torch.ones((1, 4, 4), dtype=torch.float64)
        with pytest.raises(_lib.GnnglsHipError):
            ops.aco(D, D, ants=2, iters=1)


def test_torch_op_has_a_shape_function():
    import torch

    import gnngls_amd.torch_ops  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        D = torch.empty((3, 7, 7), dtype=torch.float64, device="cuda")
        out = torch.ops.gnngls.aco(D, D, 5, 4, 0, 0.1, 0.0, 0, True, 9, None, None, None, None)
        shapes = [tuple(o.shape) for o in out]
        assert shapes == [(3, 8), (3,), (3, 7, 7), (3,), (3,), (3, 4), (3, 5, 8), (3, 5)]
        assert [o.dtype for o in out] == [torch.int32, torch.float64, torch.float64, torch.int32, torch.int32, torch.float64, torch.int32,
                                          torch.float64]
    with pytest.raises((NotImplementedError, RuntimeError)):                   # HIP key only: no CPU kernel behind the op
        z = torch.zeros((1, 4, 4), dtype=torch.float64)
        torch.ops.gnngls.aco(z, z, 2, 1, 0, 0.1, 0.0, 0, True, 0, None, None, None, None)


# ---- sanity of the definition -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [20, 50])
def test_the_colony_improves_on_its_first_iteration(n):
    rng = np.random.default_rng(1000 + n)
    for _ in range(2):
        D = euclid(rng, n)
        r = host.aco(D, inverse_square(D), ants=16, iters=60, rho=0.1, seed=0)
        print(f"n={n}: first iteration {r.trace[0]:.4f}, best {r.best_cost:.4f} ({100 * (1 - r.best_cost / r.trace[0]):.1f} % below)")
        assert r.status == 0 and r.iters_done == 60
        assert r.best_cost < r.trace[0]
        assert sorted(r.best_tour[:-1]) == list(range(n)) and r.best_tour[0] == r.best_tour[-1] == 0
        assert bits(tour_cost(r.best_tour, D)) == bits(r.best_cost) and r.best_cost == min(r.trace)
