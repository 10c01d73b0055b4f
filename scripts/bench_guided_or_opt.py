#!/usr/bin/env python
"""Measures guided local search over 2-opt and Or-opt (ops.guided_or_opt: guided_or_opt_kernel in oropt_kernels.hip) against the
persistent search kernel (ops.gls_run) on the instances bench.py searches, on one GPU.

    python scripts/bench_guided_or_opt.py [--out profiles/guided_or_opt.json] [--shapes 100x1024,200x256] [--iters 10,100,1000]
                                          [--time_iters 10] [--large_shapes 500x8,1000x4] [--large_iters 2]

Per shape of --shapes (the leading instances of block 0 of the seeded test set: same generator and seed as bench.py), from the
nearest-neighbour start, guided by the distances (guides = ("weight",)), 20 moves per perturbation:

1. device time -- HIP events on the stream, warm-up first, median of --repeats calls -- of --time_iters outer iterations of
   ops.guided_or_opt at max_seg 1 (no reversal) and 3 (reversal on) and of ops.gls_run(max_outer_iters=K) on the same load, the
   three calls ALTERNATED inside every repeat.  At max_seg=1 without reversal the two kernels walk the same trajectory: the script
   ASSERTS equal best tours and equal best costs in the run before it reports a time.
2. at every K of --iters: the mean gap of the best tours against the best-known lengths of bench_data/ at max_seg 1 and 3, the run
   timed once with events, the moves and penalisations per iteration and the runs a cap ended; next to it the mean gap of
   solve_batch(guides=("weight",), budget="per_batch", time_limit=<that run's device time>) on the same instances.  ONE wall-clock
   run per solve_batch cell: a cell carries the run-to-run spread of a wall-clock search, which this script does not measure.

Per shape of --large_shapes (uniform instances drawn here, no best-known lengths): device time of --large_iters iterations at
max_seg 1 and 3 against ops.gls_run on the global-memory store, with the same assertion.

No threshold: the cells are recorded as measured.  "Richer operators in the penalty loop are no lever" is a result.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from bench import instance_range, load_best_known  # noqa: E402
from bench_or_opt import alternated_ms, shapes_of  # noqa: E402
from gnngls_amd import ops, pipeline  # noqa: E402

PM = 20
SETTINGS = {"seg1": (1, False), "seg3": (3, True)}


def gap_pct(cost, bk):
    return float(((cost / bk - 1) * 100).mean())


def assert_same_as_gls_run(init, cost, D, guides, K):
    """max_seg=1, reverse=False against gls_run(max_outer_iters=K): equal best tours and best costs, or the script stops."""
    r = ops.guided_or_opt(init, cost, D, guides, K, perturbation_moves=PM, max_seg=1, reverse=False)
    g = ops.gls_run(D, guides, init, cost, perturbation_moves=PM, max_outer_iters=K)
    assert not r.status.any() and not g.status.any(), "a cap or a search status ended a run of the equality check"
    assert torch.equal(r.best_tour, g.best_tour) and torch.equal(r.best_cost.view(torch.int64), g.best_cost.view(torch.int64)), \
        f"guided_or_opt(max_seg=1, reverse=False) and gls_run(max_outer_iters={K}) returned different best tours or costs"
    return True


def timed_pair(init, cost, D, guides, K, warmup, repeats):
    same = assert_same_as_gls_run(init, cost, D, guides, K)
    fns = {f"guided_or_opt_{name}": (lambda s=s: ops.guided_or_opt(init, cost, D, guides, K, perturbation_moves=PM, max_seg=s[0], reverse=s[1]))
           for name, s in SETTINGS.items()}
    fns["gls_run"] = lambda: ops.gls_run(D, guides, init, cost, perturbation_moves=PM, max_outer_iters=K)
    t = alternated_ms(fns, warmup, repeats)
    t["outer_iters"] = K
    t["same_best_as_gls_run"] = same
    t["seg1_over_gls_run"] = t["guided_or_opt_seg1"]["device_ms_median"] / t["gls_run"]["device_ms_median"]
    t["seg3_over_seg1"] = t["guided_or_opt_seg3"]["device_ms_median"] / t["guided_or_opt_seg1"]["device_ms_median"]
    return t


def once_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = fn()
    b.record()
    b.synchronize()
    return r, a.elapsed_time(b)


def measure(D, bk, iters, time_iters, warmup, repeats):
    init = ops.nearest_neighbor(D)
    cost = ops.tour_cost(init, D)
    guides = D[None].contiguous()
    pipeline.solve_batch(D, guides=("weight",), time_limit=0.02, budget="per_batch")       # warm-up of the search path
    out = {"nearest_neighbor_gap_pct": gap_pct(cost.cpu().numpy(), bk), "device_time": timed_pair(init, cost, D, guides, time_iters, warmup, repeats),
           "quality": []}
    for K in iters:
        row = {"outer_iters": K, "same_best_as_gls_run": assert_same_as_gls_run(init, cost, D, guides, K)}
        for name, (seg, rev) in SETTINGS.items():
            r, ms = once_ms(lambda: ops.guided_or_opt(init, cost, D, guides, K, perturbation_moves=PM, max_seg=seg, reverse=rev))
            s = pipeline.solve_batch(D, guides=("weight",), time_limit=ms / 1e3, budget="per_batch")
            row[name] = {"device_ms_once": ms, "mean_gap_pct": gap_pct(r.best_cost.cpu().numpy(), bk),
                         "moves_per_iter": float(r.moves.double().mean() / max(K, 1)), "steps_per_iter": float(r.steps.double().mean() / max(K, 1)),
                         "capped": int((r.status != 0).sum()),
                         "solve_batch_equal_time": {"time_limit_s": ms / 1e3, "mean_gap_pct": gap_pct(s.best_cost.cpu().numpy(), bk),
                                                    "search_s": s.timing["search_s"], "chunks": s.timing["chunks"],
                                                    "mean_outer_iters": float(s.outer_iters.double().mean())}}
        out["quality"].append(row)
    return out


def measure_large(n, B, K, seed, warmup, repeats):
    from gnngls_amd.synthetic import random_instances
    D = torch.from_numpy(random_instances(np.random.default_rng(seed + n), B, n)[0]).cuda()
    init = ops.nearest_neighbor(D)
    cost = ops.tour_cost(init, D)
    return {"n": n, "instances": B, "instances_from": f"random_instances(default_rng({seed} + n), B, n)",
            "gls_run_store": "global memory" if ops.gls_resident_capacity(n) == 0 else "LDS-resident",
            "device_time": timed_pair(init, cost, D, D[None].contiguous(), K, warmup, repeats)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "guided_or_opt.json"))
    ap.add_argument("--shapes", default="100x1024,200x256", help="comma-separated n x instances")
    ap.add_argument("--iters", default="10,100,1000", help="comma-separated outer-iteration counts of the quality cells")
    ap.add_argument("--time_iters", type=int, default=10, help="outer iterations of the timed calls")
    ap.add_argument("--large_shapes", default="500x8,1000x4", help="comma-separated n x instances beyond the LDS-resident stores ('' = none)")
    ap.add_argument("--large_iters", type=int, default=2)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error("--repeats must be >= 5 (medians)")
    iters = [int(k) for k in args.iters.split(",") if k]
    res = {"command": f"python scripts/bench_guided_or_opt.py --shapes {args.shapes} --iters {args.iters} --time_iters {args.time_iters} "
                      f"--large_shapes '{args.large_shapes}' --large_iters {args.large_iters} --seed {args.seed} --warmup {args.warmup} "
                      f"--repeats {args.repeats}", "device": torch.cuda.get_device_name(0), "seed": args.seed,
           "settings": f"guides = the distances, perturbation_moves = {PM}, default k, caps and penalties, nearest-neighbour start; seg1 = "
                       "max_seg 1 without reversal (the reference's operators), seg3 = max_seg 3 with reversal",
           "timing": f"HIP events on the stream, {args.warmup} warm-up calls, median of {args.repeats}, the calls alternated inside every "
                     "repeat; the quality cells' runs are timed once",
           "equality_check": "before every time: guided_or_opt(max_seg=1, reverse=False) and gls_run(max_outer_iters=K) returned equal best "
                             "tours and bitwise equal best costs (asserted)",
           "solve_batch_equal_time": "solve_batch(guides=('weight',), budget='per_batch', time_limit=<the run's device time>): ONE "
                                     "wall-clock run per cell",
           "shapes": [], "large": []}
    for n, B in shapes_of(args.shapes):
        D = torch.from_numpy(instance_range(args.seed, n, 0, B)).cuda()
        bk, bk_how = load_best_known(None, n, args.seed, 0, B)
        if bk is None:
            res["shapes"].append({"n": n, "instances": B, "best_known": bk_how, "quality": "unmeasured"})
            continue
        res["shapes"].append({"n": n, "instances": B, "best_known": bk_how, **measure(D, bk, iters, args.time_iters, args.warmup, args.repeats)})
    for n, B in shapes_of(args.large_shapes):
        res["large"].append(measure_large(n, B, args.large_iters, args.seed, args.warmup, args.repeats))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    brief = {}
    for s in res["shapes"] + res["large"]:
        if "device_time" not in s:
            continue
        t = s["device_time"]
        b = brief[f"tsp{s['n']}x{s['instances']}"] = {
            "K": t["outer_iters"], "ms": {k: round(v["device_ms_median"], 3) for k, v in t.items() if isinstance(v, dict)},
            "same_best_as_gls_run": t["same_best_as_gls_run"]}
        for row in s.get("quality", []):
            b[f"K={row['outer_iters']}"] = {name: [round(row[name]["device_ms_once"], 2), round(row[name]["mean_gap_pct"], 4),
                                                   round(row[name]["solve_batch_equal_time"]["mean_gap_pct"], 4)] for name in SETTINGS}
    print(json.dumps(brief))
    return 0


if __name__ == "__main__":
    sys.exit(main())
