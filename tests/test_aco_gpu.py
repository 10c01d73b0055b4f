"""GPU checks of the MAX-MIN ant system (ops.aco: aco_kernel in aco_kernels.hip) against its NumPy definition, host.aco.

Everything but the heuristic's pow is compared as bit patterns: the best tour and its cost, the pheromone, the trace, the
completed iterations, the status and the ants of the last iteration.  Sizes sit at the lane edge (63 / 64 / 65) and inside the
2-, 4-, 8- and 16-slot builds; ant counts below, at and above the 16 wavefronts of a workgroup.
"""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from gnngls_amd import host, ops  # noqa: E402

BAD_WEIGHTS = 6


def bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.uint64)


def euclid(rng, B, n):
    pos = rng.random((B, n, 2))
    return np.ascontiguousarray(np.linalg.norm(pos[:, :, None] - pos[:, None], axis=3))


def heuristic(D):
    return host.aco_heuristic(D, 2.0, "inverse")


def uniforms(rng, B, K, R, n):
    u = rng.random((B, K, R, n - 1))
    u[0, 0, 0, :] = 0.0                                   # the ends of [0, 1)
    u[-1, -1, -1, :] = np.nextafter(1.0, 0.0)
    return u


def dev(x, dtype=torch.float64):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dtype).cuda()


def device_run(D, H, u=None, tau=None, best_tour=None, best_cost=None, **kw):
    r = ops.aco_launch(dev(D), dev(H), u=dev(u), tau=dev(tau), best_tour=dev(best_tour, torch.int32), best_cost=dev(best_cost),
                       want_trace=True, want_ants=True, **kw)
    torch.cuda.synchronize()
    return r


def check_against_host(D, H, u=None, tau=None, best_tour=None, best_cost=None, **kw):
    """Runs the batch on the device and every instance on the host; everything is compared as bits."""
    B, n, _ = D.shape
    r = device_run(D, H, u, tau, best_tour, best_cost, **kw)
    for b in range(B):
        o = host.aco(D[b], H[b], u=None if u is None else u[b], tau=None if tau is None else tau[b],
                     best_tour=None if best_tour is None or not np.isfinite(best_cost[b]) else best_tour[b],
                     best_cost=None if best_cost is None else best_cost[b], b=b, **kw)
        what = f"instance {b}"
        assert int(r.status[b]) == o.status and int(r.iters_done[b]) == o.iters_done, what
        assert np.array_equal(bits(r.tau[b].cpu().numpy()), bits(o.tau)), what
        assert bits(r.best_cost[b].item()) == bits(o.best_cost), what
        if o.best_tour is not None:
            assert r.best_tour[b].cpu().tolist() == o.best_tour, what
        trace = r.trace_cost[b].cpu().numpy()
        assert np.array_equal(bits(trace[:o.iters_done]), bits(np.array(o.trace, dtype=np.float64))), what
        assert np.isnan(trace[o.iters_done:]).all(), what
        if o.ant_tours is not None:
            assert np.array_equal(r.ant_tours[b].cpu().numpy(), o.ant_tours), what
            assert np.array_equal(bits(r.ant_cost[b].cpu().numpy()), bits(o.ant_cost)), what
    return r


# (n, ants, instances, iterations): every n of the issue, every ant count, host time of a case kept to a few seconds
CASES = [(3, 1, 3, 6), (3, 3, 3, 6), (3, 16, 3, 6), (3, 17, 3, 6), (3, 40, 3, 6), (4, 1, 3, 6), (4, 17, 3, 6), (5, 3, 3, 6), (5, 40, 3, 6),
         (63, 3, 2, 6), (63, 16, 2, 6), (64, 17, 2, 6), (65, 1, 2, 6), (65, 40, 2, 6), (100, 3, 2, 6), (100, 16, 2, 6), (100, 40, 2, 6), (129, 1, 2, 6), (129, 17, 2, 6),
         (257, 3, 2, 2), (257, 17, 2, 2), (257, 40, 2, 2)]


@pytest.mark.parametrize("n,R,B,K", CASES)
def test_device_equals_the_host_definition(n, R, B, K):
    rng = np.random.default_rng(1000 * n + R)
    D = euclid(rng, B, n)
    H = heuristic(D)
    for spread, gb in ((True, 0), (False, 2)) if n > 5 else ((True, 0), (False, 2), (True, 2), (False, 0)):
        r = check_against_host(D, H, uniforms(rng, B, K, R, n), ants=R, iters=K, rho=0.1, gb_every=gb, spread_starts=spread)
        assert (r.status == 0).all() and (r.iters_done == K).all()


@pytest.mark.parametrize("n", [600, 1024])
def test_large_instances(n):
    rng = np.random.default_rng(n)
    D = euclid(rng, 1, n)
    check_against_host(D, heuristic(D), uniforms(rng, 1, 2, 2, n), ants=2, iters=2, rho=0.1, gb_every=2, spread_starts=True)


@pytest.mark.parametrize("n,R", [(5, 3), (65, 17), (129, 40), (257, 4)])
def test_walks_are_the_samplers(n, R):
    """The scan, running-sum and pick code carried over into aco_kernels.hip is pinned to sampling_kernels.hip."""
    rng = np.random.default_rng(n)
    B = 2
    D = euclid(rng, B, n)
    H, tau = dev(heuristic(D)), dev(rng.uniform(0.5, 2.0, size=(B, n, n)))
    u = dev(uniforms(rng, B, 1, R, n))
    tours, status = ops.sample_nn_tours(tau * H, R, depot=0, invert=False, u=u[:, 0].contiguous())
    r = ops.aco_launch(dev(D), H, ants=R, iters=1, spread_starts=False, u=u, tau=tau.clone(), want_ants=True)
    torch.cuda.synchronize()
    assert (status == 0).all() and torch.equal(r.ant_tours, tours)
    cost = torch.stack([ops.tour_cost(tours[:, a].contiguous(), dev(D)) for a in range(R)], dim=1)
    assert np.array_equal(bits(r.ant_cost.cpu().numpy()), bits(cost.cpu().numpy()))


def test_philox_stream_two():
    rng = np.random.default_rng(7)
    B, n, R, K, iter0, seed = 3, 20, 5, 3, 4, 2024
    D = euclid(rng, B, n)
    H = heuristic(D)
    kw = dict(ants=R, iters=K, iter0=iter0, rho=0.1, seed=seed)
    drawn = check_against_host(D, H, **kw)                                     # host.aco draws instance b's stream itself
    u = host.philox_uniforms(seed, B, K * R, n - 1, k0=iter0 * R, c3=2).reshape(B, K, R, n - 1)
    given = device_run(D, H, u, **kw)
    assert torch.equal(drawn.tau.view(torch.int64), given.tau.view(torch.int64)) and torch.equal(drawn.ant_tours, given.ant_tours)
    other = device_run(D, H, host.philox_uniforms(seed, B, K * R, n - 1, k0=iter0 * R, c3=0).reshape(B, K, R, n - 1), **kw)
    assert not torch.equal(other.ant_tours, given.ant_tours)


def test_chaining_is_the_longer_run():
    rng = np.random.default_rng(8)
    B, n, R = 2, 30, 5
    D = euclid(rng, B, n)
    H = heuristic(D)
    kw = dict(ants=R, rho=0.1, gb_every=2, seed=5)
    whole = device_run(D, H, iters=7, **kw)
    a = device_run(D, H, iters=3, **kw)
    z = ops.aco(dev(D), dev(H), iters=4, iter0=3, tau=a.tau, best_tour=a.best_tour, best_cost=a.best_cost, want_trace=True, want_ants=True, **kw)
    assert torch.equal(z.tau.view(torch.int64), whole.tau.view(torch.int64)) and torch.equal(z.best_tour, whole.best_tour)
    assert torch.equal(z.best_cost.view(torch.int64), whole.best_cost.view(torch.int64)) and torch.equal(z.ant_tours, whole.ant_tours)
    assert torch.equal(torch.cat([a.trace_cost, z.trace_cost], dim=1).view(torch.int64), whole.trace_cost.view(torch.int64))
    assert z.tau.data_ptr() == a.tau.data_ptr()                                # tau is updated in place


def test_invariants_of_one_run():
    rng = np.random.default_rng(9)
    B, n, rho = 2, 100, 0.1
    D, H = dev(euclid(rng, B, n)), None
    H = ops.aco_heuristic(D, 2.0, "inverse")
    D0, H0 = D.clone(), H.clone()
    r = ops.aco(D, H, ants=16, iters=20, rho=rho, want_trace=True)
    torch.cuda.synchronize()
    assert torch.equal(ops.tour_cost(r.best_tour, D).view(torch.int64), r.best_cost.view(torch.int64))
    for b in range(B):
        t = r.best_tour[b].cpu().tolist()
        assert t[0] == t[-1] == 0 and sorted(t[:-1]) == list(range(n))
    assert torch.equal(r.trace_cost.min(dim=1).values, r.best_cost)
    assert torch.equal(r.tau.view(torch.int64), r.tau.transpose(1, 2).contiguous().view(torch.int64))
    tau_max = (1.0 / (rho * r.best_cost))[:, None, None]
    tau_min = tau_max * (1.0 / (2 * n))
    off = ~torch.eye(n, dtype=torch.bool, device=D.device)
    assert ((r.tau >= tau_min) & (r.tau <= tau_max))[:, off].all()
    assert torch.equal(D.view(torch.int64), D0.view(torch.int64)) and torch.equal(H.view(torch.int64), H0.view(torch.int64))


def test_constant_costs_keep_the_first_tour():
    rng = np.random.default_rng(10)
    B, n, R, K = 2, 10, 4, 3
    D = np.ascontiguousarray(np.broadcast_to(np.ones((n, n)) - np.eye(n), (B, n, n)))
    H = np.ones((B, n, n))
    u = uniforms(rng, B, K, R, n)
    first = device_run(D, H, u[:, :1], ants=R, iters=1, spread_starts=False)
    r = check_against_host(D, H, u, ants=R, iters=K, spread_starts=False)
    assert torch.equal(first.best_tour, first.ant_tours[:, 0]) and torch.equal(r.best_tour, first.best_tour)      # ant 0, iteration 0
    assert (r.trace_cost == float(n)).all() and not torch.equal(r.ant_tours[:, 0], r.best_tour)


def test_min_ratio_one_pins_tau_to_tau_max():
    rng = np.random.default_rng(11)
    B, n = 2, 40
    D = euclid(rng, B, n)
    r = check_against_host(D, heuristic(D), ants=6, iters=4, rho=0.2, min_ratio=1.0, seed=3)
    tau_max = (1.0 / (0.2 * r.best_cost))[:, None, None].expand(B, n, n)
    off = ~torch.eye(n, dtype=torch.bool, device=r.tau.device)
    assert torch.equal(r.tau[:, off].view(torch.int64), tau_max[:, off].contiguous().view(torch.int64))


def test_bad_weights_end_one_instance_only():
    rng = np.random.default_rng(12)
    B, n, R, K = 3, 70, 5, 4
    D = euclid(rng, B, n)
    H = heuristic(D)
    H[1, 9, :] = np.nan
    tau = rng.uniform(0.5, 1.5, size=(B, n, n))
    r = check_against_host(D, H, uniforms(rng, B, K, R, n), tau=tau, ants=R, iters=K)
    assert r.status.cpu().tolist() == [0, BAD_WEIGHTS, 0] and r.iters_done.cpu().tolist() == [K, 0, K]
    assert np.array_equal(bits(r.tau[1].cpu().numpy()), bits(tau[1])) and torch.isinf(r.best_cost[1]) and torch.isnan(r.trace_cost[1]).all()
    with pytest.raises(ValueError, match="no probabilities"):
        ops.aco(dev(D), dev(H), ants=R, iters=K)


def test_trace_stays_nan_beyond_an_early_end():
    """Column 3 of H is zero, so node 3 is visited last and its NaN row is never read -- until the single ant STARTS there, in
    iteration 3: the run ends with three completed iterations and the rest of the NaN-filled trace untouched."""
    rng = np.random.default_rng(13)
    B, n, K = 2, 5, 6
    D = euclid(rng, B, n)
    H = heuristic(D)
    H[0, :, 3] = 0.0
    H[0, 3, :] = np.nan
    r = check_against_host(D, H, uniforms(rng, B, K, 1, n), ants=1, iters=K, spread_starts=True)
    assert r.iters_done.cpu().tolist() == [3, K] and r.status.cpu().tolist() == [BAD_WEIGHTS, 0]
    trace = r.trace_cost[0].cpu().numpy()
    assert np.isfinite(trace[:3]).all() and np.isnan(trace[3:]).all() and torch.isfinite(r.best_cost[0])


def test_heuristic_matches_the_host():
    rng = np.random.default_rng(14)
    G = euclid(rng, 3, 33)
    A = rng.normal(size=(3, 33, 33))
    for x, kind, beta in ((G, "inverse", 2.0), (G, "shifted", 1.5), (A, "shifted", 2.0)):
        got = ops.aco_heuristic(dev(x), beta, kind).cpu().numpy()
        assert np.allclose(got, host.aco_heuristic(x, beta, kind), rtol=1e-12, atol=0.0)
    init = ops.aco_init_tau(dev(G), 0.1).cpu().numpy()
    for b in range(3):
        assert np.array_equal(bits(init[b]), bits(host.aco_init_tau(G[b], 0.1)))
