"""CPU checks of the sampled nearest-neighbour walks (gnngls_sample_nn_tours; reference algorithms.py:21-64).

* A NumPy restatement of the walk as include/gnngls_hip.h defines it (kept here; the GPU tests import it as their oracle):
  the inf rule, the all-zero rule, inversion, the cases np.random.choice refuses, the fixed summation order and the draw --
  and of the generator, Philox4x32-10 with counter (b, r, step, 0), checked against the published known-answer vectors.
* The law: tests/golden/pnn_law_n6.npz holds how often the REFERENCE's probabilistic_nearest_neighbour returned each of the 120
  tours of one 6-node instance in 20,000 calls (tests/golden/make_pnn_fixtures.py).  Every tour's exact probability under the
  definition is the product of its steps' p_j / total; the reference's counts must pass a chi-square test against it.
* The symbol is exported with a ctypes signature, the host-side argument checks answer before any device work, the ABI version
  did not move, and the Python surfaces have the signatures the reference's callers expect.

The summation order (include/gnngls_hip.h): node j sits on lane j % 64, slot j / 64, a node that is no candidate adds +0.0; per
slot an inclusive doubling scan over the 64 lanes (rounds d = 1, 2, .., 32: lane l >= d adds what lane l - d held before the
round); running sum of j = base_s + scan_s[j % 64], base_0 = +0.0, base_{s+1} = base_s + scan_s[63]; total = the last base.
"""
import ctypes
import inspect
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
LAW_FIXTURE = os.path.join(GOLDEN, "pnn_law_n6.npz")
BAD_WEIGHTS = 6
LANES = 64
M32 = np.uint64(0xFFFFFFFF)


# ---- the restatement ---------------------------------------------------------------------------------------------------------
def lane_scan(v):
    """Inclusive doubling (Hillis-Steele) scan of 64 fp64 values."""
    v = np.array(v, dtype=np.float64)
    for d in (1, 2, 4, 8, 16, 32):
        old = v.copy()
        v[d:] = old[d:] + old[:-d]
    return v


def running_sums(p):
    """p [n] fp64, +0.0 where the node is no candidate -> (running sum of every node [n], total)."""
    n = len(p)
    slots = (n + LANES - 1) // LANES
    padded = np.zeros(slots * LANES, dtype=np.float64)
    padded[:n] = p
    run = np.empty_like(padded)
    base = np.float64(0.0)
    for s in range(slots):
        c = lane_scan(padded[LANES * s:LANES * (s + 1)])
        run[LANES * s:LANES * (s + 1)] = base + c
        base = base + c[LANES - 1]
    return run[:n], base


def step_weights(g, cand, invert):
    """One step's p (0.0 outside the candidates) after the inf rule, the all-zero rule and inversion, or None where
    np.random.choice would raise; with it the running sums and the total."""
    with np.errstate(all="ignore"):
        p = np.where(cand, g, 0.0)
        is_inf = cand & np.isinf(g)
        if is_inf.any():                                   # algorithms.py:34-36
            p = np.where(is_inf, 1.0, 0.0)
        if running_sums(p)[1] == 0:                        # algorithms.py:39-40
            p = np.where(cand, 1.0, 0.0)
        if invert:                                         # algorithms.py:43-44
            p = np.where(cand, np.divide(1.0, p, where=cand, out=np.zeros_like(p)), 0.0)
        pc = p[cand]
        if np.isnan(pc).any() or (pc < 0).any() or np.isinf(pc).any():
            return None
        run, total = running_sums(p)
        if not (np.isfinite(total) and total > 0):
            return None
    return p, run, total


def restated_walk(W, depot, invert, u):
    """W [n,n] fp64, u [n-1] -> the closed tour (list), or None for a walk that meets bad weights."""
    n = W.shape[0]
    cand = np.ones(n, dtype=bool)
    cand[depot] = False
    tour, cur = [depot], depot
    for s in range(n - 1):
        w = step_weights(W[cur], cand, invert)
        if w is None:
            return None
        p, run, total = w
        x = np.float64(u[s]) * total
        live = cand & (p > 0)
        over = np.flatnonzero(live & (run > x))
        cur = int(over[0]) if len(over) else int(np.flatnonzero(live)[-1])
        cand[cur] = False
        tour.append(cur)
    return tour + [depot]


def restated_walks(W, depot, invert, u):
    """W [B,n,n], u [B,R,n-1] -> (tours [B,R,n+1] int32, status [B,R] int32) as the device returns them."""
    B, n, _ = W.shape
    R = u.shape[1]
    tours = np.full((B, R, n + 1), -1, dtype=np.int32)
    status = np.zeros((B, R), dtype=np.int32)
    for b in range(B):
        for r in range(R):
            t = restated_walk(W[b], depot, invert, u[b, r])
            if t is None:
                status[b, r] = BAD_WEIGHTS
            else:
                tours[b, r] = t
    return tours, status


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on uint64 arrays that hold 32-bit words -> the four output words."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) for c in (c0, c1, c2, c3))
    k0, k1 = np.uint64(k0), np.uint64(k1)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2       # 32 x 32 bits: no overflow of 64
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return c0, c1, c2, c3


def philox_uniforms(seed, B, R, steps, b0=0, r0=0):
    """u[b,r,s] of the device generator for instances b0 .. b0+B-1 and runs r0 .. r0+R-1: [B,R,steps] fp64 in [0,1)."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    b, r, s = np.meshgrid(np.arange(b0, b0 + B, dtype=np.uint64), np.arange(r0, r0 + R, dtype=np.uint64),
                          np.arange(steps, dtype=np.uint64), indexing="ij")
    o0, o1, _, _ = philox4x32_10(b, r, s, np.zeros_like(b), seed & 0xFFFFFFFF, seed >> 32)
    return (((o0 << np.uint64(32)) | o1) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def tour_probability(W, tour, invert):
    """The exact probability of a closed tour under the definition: the product of p_j / total over its steps."""
    n = W.shape[0]
    cand = np.ones(n, dtype=bool)
    cand[tour[0]] = False
    prob = 1.0
    for cur, nxt in zip(tour[:-2], tour[1:-1]):
        p, _, total = step_weights(W[cur], cand, invert)
        prob *= p[nxt] / total
        cand[nxt] = False
    return prob


def all_tours(n, depot=0):
    rest = [j for j in range(n) if j != depot]
    return [[depot] + list(perm) + [depot] for perm in itertools.permutations(rest)]


def chi_square(counts, probs):
    expected = probs * counts.sum()
    return float(((counts - expected) ** 2 / expected).sum())


def chi_square_bound(dof):
    return dof + 5.0 * np.sqrt(2.0 * dof)       # five standard deviations of the statistic under the null hypothesis


# ---- the restatement on a hand case --------------------------------------------------------------------------------------------
HAND = np.array([[0.0, 1.0, 2.0, 4.0, 4.0],
                 [1.0, 0.0, 1.0, 3.0, 2.0],
                 [2.0, 1.0, 0.0, 1.0, 5.0],
                 [4.0, 3.0, 1.0, 0.0, 2.0],
                 [4.0, 2.0, 5.0, 2.0, 0.0]])


def test_scan_is_a_prefix_sum_and_total_is_the_last_base():
    rng = np.random.default_rng(0)
    small = np.arange(1, 65, dtype=np.float64)                  # integers: every order gives the exact prefix sums
    assert np.array_equal(lane_scan(small), np.cumsum(small))
    p = rng.integers(0, 9, size=200).astype(np.float64)
    run, total = running_sums(p)
    assert np.array_equal(run, np.cumsum(p)) and total == p.sum()
    q = rng.random(130)
    run, total = running_sums(q)
    assert np.allclose(run, np.cumsum(q), rtol=1e-14) and not np.array_equal(run, np.cumsum(q))     # another order, other bits


def test_hand_case_draw_rule():
    # from node 0 with invert=False the candidates 1..4 weigh 1, 2, 4, 4: running sums 1, 3, 7, 11
    p, run, total = step_weights(HAND[0], np.array([False, True, True, True, True]), False)
    assert run.tolist() == [0.0, 1.0, 3.0, 7.0, 11.0] and total == 11.0
    first = lambda u: restated_walk(HAND, 0, False, [u, 0.0, 0.0, 0.0])[1]      # noqa: E731
    assert first(0.0) == 1 and first(0.999 / 11) == 1
    assert first(1.0 / 11) == 2                                  # x == the running sum of node 1: not exceeded -> the next node
    assert first(2.999 / 11) == 2 and first(3.0 / 11) == 3 and first(7.0 / 11) == 4
    assert first(np.nextafter(1.0, 0.0)) == 4
    # invert: 1/1, 1/2, 1/4, 1/4 -> running sums 1, 1.5, 1.75, 2
    p, run, total = step_weights(HAND[0], np.array([False, True, True, True, True]), True)
    assert run.tolist() == [0.0, 1.0, 1.5, 1.75, 2.0] and total == 2.0
    t = restated_walk(HAND, 0, True, [0.6, 0.0, 0.0, 0.0])       # x = 1.2 -> node 2; then always the first candidate
    assert t == [0, 2, 1, 3, 4, 0]
    t = restated_walk(HAND, 4, True, [0.0, 0.0, 0.0, 0.0])
    assert t == [4, 0, 1, 2, 3, 4]


def test_hand_case_inf_rule():
    W = HAND.copy()
    W[0, 3] = W[3, 0] = np.inf
    W[0, 4] = W[4, 0] = -np.inf
    cand = np.array([False, True, True, True, True])
    p, run, total = step_weights(W[0], cand, False)
    assert p.tolist() == [0.0, 0.0, 0.0, 1.0, 1.0] and total == 2.0            # algorithms.py:34-36: both infinities count
    assert restated_walk(W, 0, False, [0.49, 0, 0, 0])[1] == 3 and restated_walk(W, 0, False, [0.5, 0, 0, 0])[1] == 4
    assert step_weights(W[0], cand, True) is None                              # 1 / 0 = inf: np.random.choice raises
    only_inf = np.array([False, False, False, True, True])
    assert step_weights(W[0], only_inf, True)[0].tolist() == [0.0, 0.0, 0.0, 1.0, 1.0]     # every candidate infinite: 1 / 1


def test_hand_case_all_zero_rule():
    W = HAND.copy()
    W[0, :] = 0.0
    cand = np.array([False, True, True, False, True])
    for invert in (False, True):                                               # algorithms.py:39-40, then 1 / 1
        p, run, total = step_weights(W[0], cand, invert)
        assert p.tolist() == [0.0, 1.0, 1.0, 0.0, 1.0] and run.tolist() == [0.0, 1.0, 2.0, 2.0, 3.0] and total == 3.0
    W[0, 1] = -0.0
    assert step_weights(W[0], cand, True)[0].tolist() == [0.0, 1.0, 1.0, 0.0, 1.0]          # a sum of zeros of any sign is 0
    # a zero weight that is never the pick: node 2 has p = 0, x lands exactly on the running sum it shares with node 1
    W = HAND.copy()
    W[0, 2] = 0.0
    assert restated_walk(W, 0, False, [1.0 / 9, 0, 0, 0])[1] == 3


def test_hand_case_bad_weights():
    cand = np.array([False, True, True, True, True])
    for bad, invert in ((0.0, True), (np.nan, True), (np.nan, False), (-1.0, False), (-1.0, True), (-0.0, True)):
        W = HAND.copy()
        W[0, 2] = bad
        assert step_weights(W[0], cand, invert) is None, (bad, invert)
        assert restated_walk(W, 0, invert, [0.5] * 4) is None
        tours, status = restated_walks(W[None], 0, invert, np.full((1, 2, 4), 0.5))
        assert (status == BAD_WEIGHTS).all() and (tours == -1).all()
    W = HAND.copy()
    W[0, 2] = 0.0                                                              # a zero without inversion is a probability of zero
    assert step_weights(W[0], cand, False) is not None
    W[3, 1] = np.nan                                                           # met only by the walks that reach node 3 before node 1
    assert restated_walk(W, 0, False, [0.99, 0.99, 0.5, 0.5]) is None
    assert restated_walk(W, 0, False, [0.0, 0.5, 0.5, 0.5]) is not None
    big = np.full((5, 5), 1e308)
    assert step_weights(big[0], cand, False) is None                           # the total overflows: p / sum is no distribution


def test_philox_known_answers():
    """The known-answer vectors of Random123 (kat_vectors, philox4x32 10)."""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, out in kat:
        assert tuple(int(x) for x in philox4x32_10(*ctr, *key)) == out
    u = philox_uniforms(7, 3, 4, 9)
    assert u.shape == (3, 4, 9) and (u >= 0).all() and (u < 1).all() and len(np.unique(u)) == u.size
    assert np.array_equal(philox_uniforms(7, 1, 1, 9, b0=2, r0=3)[0, 0], u[2, 3])
    big = philox_uniforms(1, 1, 2000, 50)
    assert abs(big.mean() - 0.5) < 5 * np.sqrt(1 / 12 / big.size)


# ---- the law fixture ---------------------------------------------------------------------------------------------------------
def test_reference_counts_follow_the_definitions_law():
    z = np.load(LAW_FIXTURE)
    W, depot, calls = z["W"], int(z["depot"]), int(z["calls"])
    assert W.shape == (6, 6) and np.array_equal(W, W.T) and calls == 20000
    off = W[~np.eye(6, dtype=bool)]
    assert (off >= 1.0).all() and (off <= 2.0).all()
    tours = all_tours(6, depot)
    assert z["tours"].tolist() == tours and len(tours) == 120
    for invert, counts in ((True, z["counts_invert"]), (False, z["counts_plain"])):
        assert counts.shape == (120,) and counts.sum() == calls
        probs = np.array([tour_probability(W, t, invert) for t in tours])
        assert abs(probs.sum() - 1.0) < 1e-12
        assert (probs * calls >= 5.0).all()                     # every expected count supports the chi-square approximation
        stat = chi_square(counts.astype(np.float64), probs)
        print(f"invert={invert}: chi-square {stat:.1f} (dof 119, bound {chi_square_bound(119):.1f})")
        assert stat < chi_square_bound(119)
    # the two laws are told apart by the same statistic: the test has power
    wrong = np.array([tour_probability(W, t, False) for t in tours])
    assert chi_square(z["counts_invert"].astype(np.float64), wrong) > chi_square_bound(119)
    assert os.path.getsize(LAW_FIXTURE) < (1 << 20)


# ---- the C ABI without a GPU -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from gnngls_amd import _lib, build
    build.build()
    return _lib.load()


def test_entry_exported_with_signature(lib):
    from gnngls_amd import _lib
    raw = ctypes.CDLL(_lib.SO)
    assert hasattr(raw, "gnngls_sample_nn_tours") and "gnngls_sample_nn_tours" in _lib.SIGNATURES
    args = lib.gnngls_sample_nn_tours.argtypes
    assert len(args) == 11 and args[6] is ctypes.c_uint64
    assert lib.gnngls_abi_version() == 4
    header = open(os.path.join(ROOT, "include", "gnngls_hip.h")).read()
    for word in ("gnngls_sample_nn_tours(", "GNNGLS_SAMPLE_BAD_WEIGHTS 6", "GNNGLS_SAMPLE_MAX_N 1024", "algorithms.py:21-50",
                 "Summation order", "Philox4x32-10"):
        assert word in header, word
    assert "GNNGLS_PROF_ONE_TREE_BOUND, GNNGLS_PROF_KINDS" in header           # no new profile kind


def test_argument_checks_answer_before_any_device_work(lib):
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    call = lambda W, B, n, R, depot, u, tours, status: lib.gnngls_sample_nn_tours(W, B, n, R, depot, 1, 0, u, tours, status, None)  # noqa: E731
    hostile = [
        ((p, 1, 2, 1, 0, None, p, p), -1, b"n=2"),
        ((p, 1, 1025, 1, 0, None, p, p), -3, b"n=1025"),
        ((p, 1, 5, 0, 0, None, p, p), -1, b"R=0"),
        ((p, 1, 5, -3, 0, None, p, p), -1, b"R=-3"),
        ((p, 1, 5, 1, -1, None, p, p), -1, b"depot=-1"),
        ((p, 1, 5, 1, 5, None, p, p), -1, b"depot=5"),
        ((p, -1, 5, 1, 0, None, p, p), -1, b"B=-1"),
        ((p, 1 << 20, 5, 1 << 20, 0, None, p, p), -1, b"walks"),
        ((None, 1, 5, 1, 0, None, p, p), -1, b"NULL"),
        ((p, 1, 5, 1, 0, None, None, p), -1, b"NULL"),
        ((p, 1, 5, 1, 0, None, p, None), -1, b"NULL"),
    ]
    for args, code, msg in hostile:
        assert call(*args) == code, args
        err = lib.gnngls_last_error()
        assert err.startswith(b"sample_nn_tours:") and msg in err, err
    assert call(None, 0, 5, 3, 0, None, None, None) == 0                       # B == 0: nothing to do


def test_python_surface_without_gpu():
    from gnngls_amd import algorithms, ops, pipeline
    assert str(inspect.signature(algorithms.probabilistic_nearest_neighbour)) == "(G, depot, guide='weight', invert=True, seed=None)"
    assert (str(inspect.signature(algorithms.best_probabilistic_nearest_neighbour))
            == "(G, depot, n_iters, guide='weight', weight='weight', seed=None)")
    assert str(inspect.signature(ops.sample_nn_tours)) == "(W, R, depot=0, invert=True, seed=0, u=None)"
    assert list(inspect.signature(ops.best_sampled_tour).parameters)[:3] == ["W", "D", "R"]
    sig = inspect.signature(pipeline.solve_batch)
    assert sig.parameters["starts"].default == 1 and sig.parameters["start_seed"].default == 0
    assert list(pipeline.INIT_TOURS) == ["nearest_neighbor", "nearest_insertion", "farthest_insertion"]
    fields = {f.name: f.default for f in pipeline.SolveResult.__dataclass_fields__.values()}
    assert fields["start_costs"] is None and fields["best_start"] is None
    assert ops.SAMPLE_BAD_WEIGHTS == BAD_WEIGHTS and ops.SAMPLE_MAX_N == 1024
    assert "out of scope" not in algorithms.__doc__ and "LAW" in algorithms.__doc__
    with pytest.raises(ValueError, match="starts=0"):
        pipeline.solve_batch(None, starts=0)
    # seed=None is ONE draw from NumPy's global stream
    np.random.seed(5)
    a = algorithms._draw_seed(None)
    after = np.random.random()
    np.random.seed(5)
    assert algorithms._draw_seed(None) == a and np.random.random() == after and algorithms._draw_seed(11) == 11


def test_cli_names_the_flags():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "test.py"), "--help"], cwd=ROOT, capture_output=True,
                         text=True, check=True).stdout
    assert "--starts" in out and "--start_seed" in out


def test_torch_op_has_a_shape_function():
    import torch

    import gnngls_amd.torch_ops  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        W = torch.empty((3, 7, 7), dtype=torch.float64, device="cuda")
        t, s = torch.ops.gnngls.sample_nn_tours(W, 5, 0, True, 9, None)
        assert t.shape == (3, 5, 8) and t.dtype == torch.int32 and s.shape == (3, 5) and s.dtype == torch.int32
        u = torch.empty((3, 5, 6), dtype=torch.float64, device="cuda")
        assert torch.ops.gnngls.sample_nn_tours(W, 5, 6, False, 0, u)[0].shape == (3, 5, 8)
    with pytest.raises((NotImplementedError, RuntimeError)):                   # HIP key only: no CPU kernel behind the op
        torch.ops.gnngls.sample_nn_tours(torch.zeros((1, 4, 4), dtype=torch.float64), 2, 0, True, 0, None)
