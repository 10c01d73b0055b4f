"""The case table of the randomised parity campaign of the per-instance search kernels -- Or-opt (scan, descent, one-to-all scan),
3-opt (scan, descent), iterated local search and guided local search over 2-opt and Or-opt -- and the CPU half of that campaign:
tests/test_search_fuzz_gpu.py imports CASES, instances() and expected() from here and compares the kernels with them bit for bit.

Inputs are the six kinds of make_case (tests/test_gls_fuzz_gpu.py) and one more, `tiny`: unit-square coordinates times 3e-7, so
that most deltas of a scan lie within a few 1e-8 of zero, inside or beside the band of np.isclose(0, delta).  Here, without a GPU:

  1. the vectorised definitions of gnngls_amd.host equal the scalar restatements of the neighbouring _cpu files (the literal loops
     that evaluate `delta < best_delta and not np.isclose(0, delta)` candidate by candidate, and the C oracle's 2-opt scans) on
     every kind, which so far they did on Euclidean and tie-heavy inputs only;
  2. every case of the table ends on the host with status 0 -- no cap ended it -- except the cases of CAPPED, which are there to
     end on one (the 3-opt descents at n = 200 and 201, whose full host descent takes minutes, and one guided run on its step
     cap); every
     `negative` instance has a positive start-tour cost (a negative one makes k negative and the penalty loop endless in the
     reference itself);
  3. every near-zero case (lattice, noisy, tiny) proves its worth: the same definition with the closeness test switched off
     (host._isclose0 always answers "not close": a kernel that ignores the rule) gives a different result in at least one compared
     field, for every such case of the table.  The second mutant, the rule replaced by `delta < -1e-8`, differs from the rule only
     for deltas in (-1.00001e-8, -1e-8): every `noisy` case of the table is caught by it too (the seeds were picked for that:
     the noise terms of that kind are multiples of those two numbers); `tiny` and `lattice` deltas land in a band 1e-13 wide only
     by accident and are not asked to.  `lattice` matrices are integers, every delta of a plain descent is exact and no rule about
     closeness can matter: that kind is given to the guided kernel only, where D + k * penalty brings the fractions.

Seeds: a slot's seed is the first of 0, 1, 2, ... for which 2. and 3. hold.  Seed 0 did for every slot but these: `negative` at
n = 5 (72: the first whose three start tours all cost more than 0), `noisy` at n = 5 for Or-opt (1) and 3-opt (2) (the seeds
before them were replaced: with so few candidates not both mutants change a result).  The tests here fail if a seed stops
satisfying its conditions.

Where the host's time goes: three_opt_descent.  One host evaluation of a case (three instances, every compared field) on one CPU
core took, slowest case per kernel: Or-opt 0.4 s (n = 129 huge), ILS 0.5 s (n = 129 tiny), guided 1.4 s (n = 33 negative: up to
900 penalty steps per run), 3-opt 0.6 - 1.8 s at n = 100, 1.8 - 2.4 s at n = 129 and 3 s at n = 200 and 201 under max_moves = 4
(nonmetric and huge at n = 129 took 3.5 - 4.6 s: that size gets the cheaper near-zero kinds).  The whole table: 28 s, this file
about 40 s.  A guided run on a `negative` instance whose start tour costs less than 0 never finishes: k < 0, and a run of
n = 129 spent its 4,000 steps in 15 s; the table holds no such instance, and beyond n = 33 no seed gives one that is not."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

from gnngls_amd import host  # noqa: E402
from test_gls_fuzz_gpu import make_case  # noqa: E402
from test_guided_or_opt_cpu import brute_or_opt_o2a, k_of  # noqa: E402
from test_or_opt_cpu import bits, random_tour  # noqa: E402
from test_or_opt_cpu import literal_a2a as literal_or_opt_a2a  # noqa: E402
from test_three_opt_cpu import literal_a2a as literal_three_opt_a2a  # noqa: E402

KINDS = ("euclid", "lattice", "noisy", "tiny", "nonmetric", "negative", "huge")
NEAR_ZERO = ("lattice", "noisy", "tiny")
B = 3                                                           # instances per case
OR_OPT_SETTINGS = [(1, False), (2, True), (3, True)]            # (max_seg, reverse)
SETTINGS = [(1, False), (3, True)]


def make(rng, n, kind):
    """-> (D, guide) of one instance: make_case's kinds, and `tiny`.  D symmetric bit for bit, the guide about half zeros."""
    if kind != "tiny":
        return make_case(rng, n, kind)
    pos = rng.random((n, 2)) * 3e-7
    D = np.sqrt(((pos[:, None] - pos[None]) ** 2).sum(-1))
    D = np.triu(D, 1)
    D = D + D.T
    g = np.maximum(rng.normal(0.0, 0.1, size=(n, n)).astype(np.float32).astype(np.float64), 0)
    g = np.triu(g, 1)
    return D, g + g.T


def instances(c):
    """-> (Ds [B,n,n], Gs [B,n,n]) of a case."""
    rng = np.random.default_rng(c["seed"])
    Ds, Gs = zip(*[make(rng, c["n"], c["kind"]) for _ in range(B)])
    return np.stack(Ds), np.stack(Gs)


def oracle():
    from oracle import gls_oracle
    gls_oracle.build()
    return gls_oracle


def starts(Ds):
    """The nearest-neighbour tours on D from node 0 and their costs, as the C oracle computes them (the GPU campaign asserts that
    the device gives these tours)."""
    go = oracle()
    tours = [go.nearest_neighbor(D) for D in Ds]
    return tours, [go.tour_cost(t, D) for t, D in zip(tours, Ds)]


def o2a_positions(n):
    return [1, n - 1, (n + 1) // 2]


def uniforms(c):
    """The explicit uniforms [B,kicks,3] of an ILS case."""
    return np.random.default_rng(c["seed"] + 77).random((B, c["kicks"], 3))


def expected(c, Ds, Gs, tours, costs):
    """The host definition of everything the campaign compares for case c, per instance: a dict of lists indexed [setting][b] (or
    [b] for 3-opt, which has no settings)."""
    n, kernel = c["n"], c["kernel"]
    out = {}
    if kernel == "or_opt":
        out["scan"] = [[host.or_opt_a2a(tours[b], Ds[b], ms, rv) for b in range(B)] for ms, rv in OR_OPT_SETTINGS]
        out["descent"] = [[host.or_opt_descent(tours[b], costs[b], Ds[b], ms, rv, c.get("max_moves")) for b in range(B)]
                          for ms, rv in OR_OPT_SETTINGS]
        # the one-to-all scan from the start tour and from the tour two descent moves leave
        two = [host.or_opt_descent(tours[b], costs[b], Ds[b], 3, True, 2)[0] for b in range(B)]
        out["o2a_tours"] = [tours, two]
        out["o2a"] = [[[[host.or_opt_o2a(ts[b], Ds[b], p, ms, rv) for b in range(B)] for p in o2a_positions(n)] for ts in (tours, two)]
                      for ms, rv in OR_OPT_SETTINGS]
    elif kernel == "three_opt":
        out["scan"] = [host.three_opt_a2a(tours[b], Ds[b]) for b in range(B)]
        out["descent"] = [host.three_opt_descent(tours[b], costs[b], Ds[b], c.get("max_moves")) for b in range(B)]
    elif kernel == "ils":
        u = uniforms(c)
        out["run"] = [[host.ils(tours[b], costs[b], Ds[b], c["kicks"], ms, rv, c.get("max_moves"), u[b]) for b in range(B)]
                      for ms, rv in SETTINGS]
    else:
        assert kernel == "guided"
        rows = []
        for ms, rv in SETTINGS:
            row = []
            for b in range(B):
                pen = np.zeros((n, n), dtype=np.int32)
                r = host.guided_or_opt(tours[b], costs[b], Ds[b], np.stack([Gs[b], Ds[b]]), c["K"], k_of(costs[b], n), pen, c["pm"], ms, rv,
                                       max_moves=c["max_moves"], max_steps=c["max_steps"])
                row.append((r, pen))
            rows.append(row)
        out["run"] = rows
    return out


def canon(x):
    """A result as a nested tuple that == compares bit for bit."""
    if isinstance(x, dict):
        return tuple((k, canon(v)) for k, v in sorted(x.items()))
    if isinstance(x, (list, tuple)):
        return tuple(canon(v) for v in x)
    if isinstance(x, np.ndarray):
        return (x.dtype.str, x.shape, x.tobytes())
    if isinstance(x, (float, np.floating)):
        return ("f", int(np.float64(x).view(np.uint64)))
    if isinstance(x, (int, np.integer)):
        return ("f", 0) if x == 0 else int(x)                   # a scan that finds nothing answers the int 0
    assert x is None, type(x)
    return None


def statuses(c, want):
    """The status of every host run of a case: 3-opt and Or-opt descents report MOVE_CAP where they applied max_moves moves."""
    k = c["kernel"]
    if k == "or_opt":
        return [6 if r[2] == c.get("max_moves") else 0 for row in want["descent"] for r in row]
    if k == "three_opt":
        return [6 if r[2] == c.get("max_moves") else 0 for r in want["descent"]]
    if k == "ils":
        return [r[4] for row in want["run"] for r in row]
    return [r[6] for row in want["run"] for r, pen in row]


def case(kernel, n, kind, seed, **kw):
    return dict(kernel=kernel, n=n, kind=kind, seed=seed, **kw)


def case_id(c):
    return f"{c['kernel']}-n{c['n']}-{c['kind']}-s{c['seed']}"


# --- the table --------------------------------------------------------------------------------------------------------------------
# sizes, each tied to code: a handful of candidates (5, 9), two and three wavefronts (17, 33), the lane loop's edge (64, 65), 100,
# the two-step arg-min (129); 3-opt: its first sixteen-wavefront size (61) and the two sides of the LDS switch-over (200, 201: under
# max_moves, like the existing large-size tests)
def _plain(kernel, **kw):
    """The slots of the three kernels without a penalty matrix: `negative` up to n = 33 only (beyond it no nearest-neighbour tour
    of that kind has a positive cost), the near-zero kinds and the badly scaled ones at every size class."""
    return [case(kernel, 5, "negative", 72, **kw), case(kernel, 5, "noisy", {"or_opt": 1, "three_opt": 2}.get(kernel, 0), **kw),
            case(kernel, 9, "negative", 0, **kw), case(kernel, 9, "tiny", 0, **kw),
            case(kernel, 17, "negative", 0, **kw), case(kernel, 17, "huge", 0, **kw),
            case(kernel, 33, "negative", 0, **kw), case(kernel, 33, "nonmetric", 0, **kw),
            case(kernel, 64, "noisy", 0, **kw), case(kernel, 64, "huge", 0, **kw),
            case(kernel, 65, "tiny", 0, **kw), case(kernel, 65, "nonmetric", 0, **kw)]


def _kicks(cases, small, large):
    return [dict(c, kicks=small if c["n"] <= 33 else large) for c in cases]


_GUIDED = dict(pm=10, max_moves=4000, max_steps=4000)           # caps that end no run but those of CAPPED
CASES = (
    _plain("or_opt") + [case("or_opt", 100, "noisy", 0), case("or_opt", 100, "nonmetric", 0), case("or_opt", 100, "euclid", 0),
                        case("or_opt", 129, "tiny", 0), case("or_opt", 129, "huge", 0)] +
    # the host's 3-opt descent is the slow one: the cheaper kinds at 129
    _plain("three_opt") + [case("three_opt", 61, "euclid", 0), case("three_opt", 61, "noisy", 0),
                           case("three_opt", 100, "noisy", 0), case("three_opt", 100, "huge", 0),
                           case("three_opt", 129, "tiny", 0), case("three_opt", 129, "noisy", 0),
                           case("three_opt", 200, "huge", 0, max_moves=4), case("three_opt", 201, "nonmetric", 0, max_moves=4)] +
    _kicks(_plain("ils") + [case("ils", 100, "noisy", 0), case("ils", 100, "nonmetric", 0), case("ils", 100, "euclid", 0),
                            case("ils", 129, "tiny", 0), case("ils", 129, "huge", 0)], 6, 4) +
    [case("guided", 5, "negative", 72, K=3, **_GUIDED), case("guided", 5, "lattice", 0, K=3, **_GUIDED),
     case("guided", 9, "negative", 0, K=3, **_GUIDED), case("guided", 9, "noisy", 0, K=3, **_GUIDED),
     case("guided", 17, "negative", 0, K=3, **_GUIDED), case("guided", 17, "tiny", 0, K=3, **_GUIDED),
     case("guided", 33, "negative", 0, K=3, **_GUIDED), case("guided", 33, "nonmetric", 0, K=3, **_GUIDED),
     case("guided", 33, "negative", 2, K=3, pm=10, max_moves=4000, max_steps=60),           # ends on the step cap
     case("guided", 64, "lattice", 0, K=3, **_GUIDED), case("guided", 64, "huge", 0, K=3, **_GUIDED),
     case("guided", 65, "noisy", 0, K=3, **_GUIDED), case("guided", 65, "nonmetric", 0, K=3, **_GUIDED),
     case("guided", 100, "tiny", 0, K=2, **_GUIDED), case("guided", 100, "nonmetric", 0, K=2, **_GUIDED),
     case("guided", 100, "euclid", 0, K=2, **_GUIDED),
     case("guided", 129, "lattice", 0, K=2, **_GUIDED), case("guided", 129, "noisy", 0, K=2, **_GUIDED),
     case("guided", 129, "huge", 0, K=2, **_GUIDED)])

# the cases that end on a cap: the two large 3-opt sizes (a full host descent there takes minutes) and one guided run
CAPPED = {"three_opt-n200-huge-s0", "three_opt-n201-nonmetric-s0", "guided-n33-negative-s2"}


# --- 1. the vectorised definitions against the scalar restatements, on every kind ---------------------------------------------------
def scalar_tours(kind, n):
    rng = np.random.default_rng(9000 + n)
    D, _ = make(rng, n, kind)
    go = oracle()
    return D, [go.nearest_neighbor(D), random_tour(rng, n)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", [7, 20, 33])
def test_or_opt_scan_and_descent_step_equal_the_literal_loop(n, kind):
    go = oracle()
    D, tours = scalar_tours(kind, n)
    found = 0
    for t in tours:
        for ms, rv in OR_OPT_SETTINGS:
            want = literal_or_opt_a2a(t, D, ms, rv)
            got = host.or_opt_a2a(t, D, ms, rv)
            assert got[1] == want[1] and bits(got[0]) == bits(want[0]), (n, kind, ms, rv, got, want)
            found += want[1] is not None
            # one descent step: the oracle's 2-opt scan first, the literal Or-opt scan when that finds nothing
            c0 = go.tour_cost(t, D)
            d2, new2, mv2 = go.two_opt_a2a(t, D)
            h2 = host.two_opt_a2a(t, D)
            assert (None if mv2 is None else tuple(mv2)) == h2[1] and bits(float(d2)) == bits(float(h2[0])), (n, kind, mv2, h2)
            step = host.or_opt_descent(t, c0, D, ms, rv, max_moves=1)
            if mv2 is not None:
                assert step[0] == new2 and bits(step[1]) == bits(c0 + d2) and step[2] == 1
            elif want[1] is not None:
                assert step[0] == host.or_opt(t, *want[1]) and bits(step[1]) == bits(c0 + want[0]) and step[2] == 1
            else:
                assert step[0] == list(t) and bits(step[1]) == bits(c0) and step[2] == 0
    assert found > 0


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", [6, 12, 20])
def test_three_opt_scan_and_descent_step_equal_the_literal_loop(n, kind):
    go = oracle()
    D, tours = scalar_tours(kind, n)
    found = 0
    for t in tours:
        want = literal_three_opt_a2a(t, D)
        got = host.three_opt_a2a(t, D)
        assert got[1] == want[1] and bits(got[0]) == bits(want[0]), (n, kind, got, want)
        found += want[1] is not None
        c0 = go.tour_cost(t, D)
        d2, new2, mv2 = go.two_opt_a2a(t, D)
        step = host.three_opt_descent(t, c0, D, max_moves=1)
        if mv2 is not None:
            assert step[0] == new2 and bits(step[1]) == bits(c0 + d2) and step[2] == 1
        elif want[1] is not None:
            assert step[0] == host.three_opt(t, *want[1]) and bits(step[1]) == bits(c0 + want[0]) and step[2] == 1
        else:
            assert step[0] == list(t) and bits(step[1]) == bits(c0) and step[2] == 0
    assert found > 0


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", [6, 13, 33])
def test_one_to_all_scans_equal_the_scalar_ones_at_every_position(n, kind):
    go = oracle()
    D, tours = scalar_tours(kind, n)
    found = 0
    for t in tours:
        for i in range(1, n):
            d, new, mv = go.two_opt_o2a(t, D, i)
            hd, hm = host.two_opt_o2a(t, D, i)
            assert bits(float(d)) == bits(float(hd)) and (None if mv is None else tuple(mv)) == hm, (n, kind, i, mv, hm)
            for ms, rv in ((2, True), (3, True)) if n < 33 else ((3, True),):
                want = brute_or_opt_o2a(t, D, i, ms, rv)
                got = host.or_opt_o2a(t, D, i, ms, rv)
                assert bits(float(want[0])) == bits(float(got[0])) and want[1] == got[1], (n, kind, i, ms, rv, want, got)
                found += got[1] is not None
            d, new, mv = go.relocate_o2a(t, D, i)
            hd, hm = host.or_opt_o2a(t, D, i, 1, False)
            assert bits(float(d)) == bits(float(hd)) and (None if mv is None else (i, 1, 0, mv[1])) == hm, (n, kind, i, mv, hm)
    assert found > 0


# --- 2. and 3. the table -----------------------------------------------------------------------------------------------------------
_want = {}


def want_of(c):
    """(Ds, Gs, tours, costs, expected) of a case, computed once."""
    key = case_id(c)
    if key not in _want:
        Ds, Gs = instances(c)
        tours, costs = starts(Ds)
        _want[key] = (Ds, Gs, tours, costs, expected(c, Ds, Gs, tours, costs))
    return _want[key]


def test_the_table_covers_what_it_says():
    ids = [case_id(c) for c in CASES]
    assert len(set(ids)) == len(ids) and 60 <= len(ids) <= 80
    for kernel in ("or_opt", "three_opt", "ils", "guided"):
        mine = [c for c in CASES if c["kernel"] == kernel]
        sizes = {c["n"] for c in mine}
        assert sizes >= {5, 9, 17, 33, 64, 65, 100, 129}, (kernel, sizes)
        if kernel == "three_opt":
            assert sizes >= {61, 200, 201}
        kinds = {c["kind"] for c in mine}
        assert kinds >= set(KINDS) - ({"lattice"} if kernel != "guided" else set()), (kernel, kinds)
        assert sum(c["kind"] == "euclid" for c in mine) == 1
    assert len(CAPPED) <= 5 and CAPPED <= set(ids)


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_case_ends_without_a_cap_and_starts_with_a_positive_cost(c):
    Ds, Gs, tours, costs, want = want_of(c)
    assert all(np.array_equal(D, D.T) for D in Ds)
    if c["kind"] == "negative":
        assert (Ds < 0).any(axis=(1, 2)).all() and min(costs) > 0, costs
    st = statuses(c, want)
    if case_id(c) in CAPPED:
        assert any(st), st
    else:
        assert not any(st), st


def mutant(c, rule):
    Ds, Gs, tours, costs, want = want_of(c)
    mp = pytest.MonkeyPatch()
    mp.setattr(host, "_isclose0", rule)
    try:
        # a descent that ignores the rule may cycle between tours of equal cost: every mutant run is capped, a few moves
        # beyond the longest run of the case (a mutant that gets that far differs in its status)
        cm = dict(c)
        if c["kernel"] == "guided":
            runs = [r for row in want["run"] for r, pen in row]
            cm["max_steps"] = min(c["max_steps"], max(r[5] for r in runs) + 8)
        else:
            runs = want["descent"] if c["kernel"] == "three_opt" else [r for row in want["descent" if c["kernel"] == "or_opt" else "run"]
                                                                       for r in row]
        cm["max_moves"] = min(c.get("max_moves", 1 << 30), max(r[4 if c["kernel"] == "guided" else 2] for r in runs) + 8)
        got = expected(cm, Ds, Gs, tours, costs)
    finally:
        mp.undo()
    return canon(got) != canon(want)


def never_close(delta):
    return np.zeros(np.shape(delta), dtype=bool) if np.ndim(delta) else False


def strictly_below_1e8(delta):
    return np.abs(delta) <= 1e-8                                # with `delta < 0`: accepted iff delta < -1e-8


@pytest.mark.parametrize("c", [c for c in CASES if c["kind"] in NEAR_ZERO], ids=case_id)
def test_near_zero_case_catches_a_kernel_without_the_closeness_rule(c):
    assert mutant(c, never_close)
    if c["kind"] == "noisy":
        assert mutant(c, strictly_below_1e8)
