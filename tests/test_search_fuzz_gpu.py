"""Randomised parity campaign of the per-instance search kernels that came after the GLS kernel -- Or-opt (all-to-all scan, descent,
one-to-all scan), 3-opt (scan, descent), iterated local search, guided local search over 2-opt and Or-opt -- against the NumPy
definitions of gnngls_amd.host, on matrices that are no well-scaled distances: deltas around np.isclose's 1e-8 threshold (noisy,
tiny, and lattice under penalties), no triangle inequality, negative entries, magnitudes of 1e7.  The case table, its instances and
the host evaluation come from tests/test_search_fuzz_cpu.py, which shows without a GPU that every near-zero case would catch a
kernel that ignores the closeness rule, and that no cap ends a run it is not meant to end.  B = 3 instances per case from the
nearest-neighbour tour on D; equality means equal tours and moves, equal bit patterns of every fp64 value, equal int32 penalties,
equal counters and statuses."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from gnngls_amd import host  # noqa: E402
from test_guided_or_opt_gpu import CAP, assert_run  # noqa: E402
from test_or_opt_cpu import bits  # noqa: E402
from test_search_fuzz_cpu import (B, CASES, OR_OPT_SETTINGS, SETTINGS, case_id, expected, instances, o2a_positions, oracle,  # noqa: E402
                                  uniforms)

MOVE_CAP = 6


def dev(x, dtype=torch.float64):
    from gnngls_amd import ops
    return ops.as_dev(np.asarray(x), dtype)


def first_mismatch(got, want):
    g, w = bits(got), bits(want)
    k = min(len(g), len(w))
    bad = np.nonzero(g[:k] != w[:k])[0]
    return f"first mismatch at move {int(bad[0]) if len(bad) else k} of {len(w)}"


def check_scan(got, rows, tours, apply, what):
    delta, move, new = (x.cpu().numpy() for x in got)
    for b, (wd, wm) in enumerate(rows):
        assert move[b].tolist() == (list(wm) if wm else [-1] * 4), (what, b, move[b].tolist(), wm)
        assert bits(delta[b]) == bits(float(wd)), (what, b, delta[b], wd)
        assert new[b].tolist() == (apply(tours[b], *wm) if wm else list(tours[b])), (what, b)


def check_descent(r, rows, max_moves, what):
    tour, cost, moves, st, trace = (x.cpu().numpy() for x in (r.tour, r.cost, r.moves, r.status, r.trace_cost))
    for b, (wt, wc, wm, wtr) in enumerate(rows):
        assert wm <= trace.shape[1]
        k = min(int(moves[b]), wm)
        assert np.array_equal(bits(trace[b, :k]), bits(wtr[:k])), (what, b, first_mismatch(trace[b, :k], wtr[:k]))
        assert int(moves[b]) == wm, (what, b, int(moves[b]), wm)
        assert tour[b].tolist() == wt, (what, b)
        assert bits(cost[b]) == bits(wc), (what, b, cost[b], wc)
        assert int(st[b]) == (MOVE_CAP if wm == max_moves else 0), (what, b, int(st[b]))
        assert not trace[b, wm:].any(), (what, b)


def check_ils(r, rows, what):
    tour, cost, moves, acc, st, trace = (x.cpu().numpy() for x in (r.tour, r.cost, r.moves, r.accepted, r.status, r.trace_cost))
    for b, w in enumerate(rows):
        ran = len(w[5])
        assert np.array_equal(bits(trace[b, :ran]), bits(w[5])), (what, b, first_mismatch(trace[b, :ran], w[5]))
        assert np.isnan(trace[b, ran:]).all(), (what, b)
        assert tour[b].tolist() == w[0], (what, b)
        assert bits(cost[b]) == bits(w[1]), (what, b, cost[b], w[1])
        assert (int(moves[b]), int(acc[b]), int(st[b])) == w[2:5], (what, b, moves[b], acc[b], st[b], w[2:5])


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_fuzz_case(c):
    from gnngls_amd import ops
    go = oracle()
    n, kernel = c["n"], c["kernel"]
    Ds, Gs = instances(c)
    D = dev(Ds)
    t = ops.nearest_neighbor(D)
    cost = ops.tour_cost(t, D)
    tours, costs = t.cpu().numpy().tolist(), cost.cpu().numpy()
    for b in range(B):
        assert tours[b] == go.nearest_neighbor(Ds[b]), b
        assert bits(costs[b]) == bits(go.tour_cost(tours[b], Ds[b])), b
    want = expected(c, Ds, Gs, tours, costs)
    cap = c.get("max_moves")
    if kernel == "or_opt":
        two = ops.or_opt_descent(t, cost, D, max_moves=2).tour
        assert two.cpu().numpy().tolist() == want["o2a_tours"][1]
        for si, (ms, rv) in enumerate(OR_OPT_SETTINGS):
            what = f"{case_id(c)} max_seg={ms} reverse={rv}"
            check_scan(ops.or_opt_best_move(t, D, ms, rv), want["scan"][si], tours, host.or_opt, what)
            check_descent(ops.or_opt_descent(t, cost, D, ms, rv, max_moves=cap, trace_cap=4 * n), want["descent"][si], cap, what)
            for ti, td in enumerate((t, two)):
                for pi, p in enumerate(o2a_positions(n)):
                    got = ops.or_opt_o2a(td, D, dev([p] * B, torch.int32), ms, rv)
                    check_scan(got, want["o2a"][si][ti][pi], want["o2a_tours"][ti], host.or_opt, f"{what} o2a tour {ti} position {p}")
    elif kernel == "three_opt":
        check_scan(ops.three_opt_best_move(t, D), want["scan"], tours, host.three_opt, case_id(c))
        check_descent(ops.three_opt_descent(t, cost, D, max_moves=cap, trace_cap=4 * n), want["descent"], cap, case_id(c))
    elif kernel == "ils":
        u = dev(uniforms(c))
        for si, (ms, rv) in enumerate(SETTINGS):
            r = ops.ils(t, cost, D, c["kicks"], ms, rv, max_moves=cap, u=u, want_trace=True)
            check_ils(r, want["run"][si], f"{case_id(c)} max_seg={ms} reverse={rv}")
    else:
        # guide 0: about half of its entries are 0, so many utilities tie at 0 and the first must win; guide 1: the distances
        g = dev(np.stack([Gs, Ds]))
        for si, (ms, rv) in enumerate(SETTINGS):
            r = ops.guided_or_opt(t, cost, D, g, c["K"], perturbation_moves=c["pm"], max_seg=ms, reverse=rv, max_moves=c["max_moves"],
                                  max_steps=c["max_steps"], trace_cap=CAP)
            assert max(w[4] for w, pen in want["run"][si]) <= CAP
            assert_run(r, want["run"][si], f"{case_id(c)} max_seg={ms} reverse={rv}")
