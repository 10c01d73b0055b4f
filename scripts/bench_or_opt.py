#!/usr/bin/env python
"""Measures the Or-opt descent (ops.or_opt_descent, oropt_kernels.hip; pipeline.solve_batch(polish="or_opt")) on the instances
bench.py searches, on one GPU.

    python scripts/bench_or_opt.py [--out profiles/or_opt.json] [--shapes 100x1024,200x256] [--polish_shapes 200x16,100x1024]

Per shape of --shapes (the leading instances of block 0 of the seeded test set: same generator and seed as bench.py), from the
nearest-neighbour start:

1. device time -- HIP events on the stream, warm-up first, median of --repeats calls -- of ops.or_opt_descent at max_seg 1 (no
   reversal) and 3 (reversal on) and of ops.gls_run(..., max_outer_iters=0) on the same load, the three calls ALTERNATED inside
   every repeat.  At max_seg=1 without reversal the new kernel and the persistent search kernel walk the same trajectory (the flag
   `same_result_as_gls_run` records that they returned the same tours and costs), so that pair compares the plain stand-alone
   kernel with the tuned one on identical work.
2. the local optimum's mean length against the best-known lengths of bench_data/ at max_seg 1 / 2 / 3 (reversal on), with the
   moves applied and the runs the move cap ended.

Per shape of --polish_shapes: solve_batch(guides=("weight",), budget="per_batch", polish="or_opt") at budgets of 0.1 / 0.3 / 1 s:
mean gap before and after the polish, the share of instances the polish moved, and timing["polish_s"] (outside the budget).  ONE
wall-clock run per cell: a cell carries the run-to-run spread of a wall-clock search, which this script does not measure.

No threshold: the cells are recorded as measured.  A polish that finds nothing on converged tours is a result.
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
from gnngls_amd import ops, pipeline  # noqa: E402

GRID_S = (0.1, 0.3, 1.0)


def alternated_ms(fns, warmup, repeats):
    """{name: (median, all)} device milliseconds of every fn of `fns`, the calls alternated inside each repeat."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    return {k: {"device_ms_median": float(np.median(v)), "device_ms_all": [float(x) for x in v]} for k, v in ms.items()}


def measure_descent(D, bk, warmup, repeats):
    init = ops.nearest_neighbor(D)
    cost = ops.tour_cost(init, D)
    out = {"device_time": alternated_ms({
        "or_opt_descent_seg1": lambda: ops.or_opt_descent(init, cost, D, 1, False),
        "gls_run_local_search": lambda: ops.gls_run(D, None, init, cost, max_outer_iters=0),
        "or_opt_descent_seg3": lambda: ops.or_opt_descent(init, cost, D, 3, True)}, warmup, repeats)}
    r1, g = ops.or_opt_descent(init, cost, D, 1, False), ops.gls_run(D, None, init, cost, max_outer_iters=0)
    t = out["device_time"]
    t["same_result_as_gls_run"] = bool(torch.equal(r1.tour, g.best_tour) and torch.equal(r1.cost, g.best_cost))
    t["seg1_over_gls_run"] = t["or_opt_descent_seg1"]["device_ms_median"] / t["gls_run_local_search"]["device_ms_median"]
    t["seg3_over_seg1"] = t["or_opt_descent_seg3"]["device_ms_median"] / t["or_opt_descent_seg1"]["device_ms_median"]
    out["local_optimum"] = {"nearest_neighbor": {"mean_gap_pct": None if bk is None else float(((cost.cpu().numpy() / bk - 1) * 100).mean())}}
    for seg in (1, 2, 3):
        r = ops.or_opt_descent(init, cost, D, seg, True)
        c = r.cost.cpu().numpy()
        out["local_optimum"][f"max_seg_{seg}"] = {"mean_length": float(c.mean()),
                                                  "mean_gap_pct": None if bk is None else float(((c / bk - 1) * 100).mean()),
                                                  "mean_moves": float(r.moves.double().mean()),
                                                  "move_cap": int((r.status == ops.STATUS_MOVE_CAP).sum())}
    return out


def measure_polish(D, bk):
    pipeline.solve_batch(D, guides=("weight",), time_limit=0.05, polish="or_opt")       # warm-up: every kernel of the path has run once
    rows = []
    for s in GRID_S:
        r = pipeline.solve_batch(D, guides=("weight",), time_limit=s, perturbation_moves=20, budget="per_batch", polish="or_opt")
        after = r.best_cost.cpu().numpy()
        before = after + r.polish_gain.cpu().numpy()
        rows.append({"budget_s": s, "mean_gap_before_pct": float(((before / bk - 1) * 100).mean()),
                     "mean_gap_after_pct": float(((after / bk - 1) * 100).mean()),
                     "share_moved": float((r.polish_gain > 0).double().mean()), "mean_gain": float(r.polish_gain.mean()),
                     "polish_s": r.timing["polish_s"], "search_s": r.timing["search_s"], "chunks": r.timing["chunks"],
                     "mean_outer_iters": float(r.outer_iters.double().mean())})
    return rows


def shapes_of(text):
    return [tuple(int(x) for x in s.split("x")) for s in text.split(",") if s]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "or_opt.json"))
    ap.add_argument("--shapes", default="100x1024,200x256", help="descent: comma-separated n x instances")
    ap.add_argument("--polish_shapes", default="200x16,100x1024", help="polish: comma-separated n x instances")
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error("--repeats must be >= 5 (medians)")
    res = {"command": f"python scripts/bench_or_opt.py --shapes {args.shapes} --polish_shapes {args.polish_shapes} --seed {args.seed} "
                      f"--warmup {args.warmup} --repeats {args.repeats}", "device": torch.cuda.get_device_name(0), "seed": args.seed,
           "timing": f"HIP events on the stream, {args.warmup} warm-up calls, median of {args.repeats}, the calls alternated inside every repeat",
           "polish_budget": "solve_batch(guides=('weight',), time_limit=s, budget='per_batch', polish='or_opt'): the polish runs after "
                            "the search, outside s; ONE wall-clock run per cell",
           "descent": [], "polish": []}
    for n, B in shapes_of(args.shapes):
        D = torch.from_numpy(instance_range(args.seed, n, 0, B)).cuda()
        bk, bk_how = load_best_known(None, n, args.seed, 0, B)
        res["descent"].append({"n": n, "instances": B, "best_known": bk_how, **measure_descent(D, bk, args.warmup, args.repeats)})
    for n, B in shapes_of(args.polish_shapes):
        D = torch.from_numpy(instance_range(args.seed, n, 0, B)).cuda()
        bk, bk_how = load_best_known(None, n, args.seed, 0, B)
        res["polish"].append({"n": n, "instances": B, "best_known": bk_how,
                              "cells": measure_polish(D, bk) if bk is not None else "unmeasured"})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    brief = {}
    for s in res["descent"]:
        t = s["device_time"]
        brief[f"descent tsp{s['n']}x{s['instances']}"] = {
            "ms": {k: round(v["device_ms_median"], 3) for k, v in t.items() if isinstance(v, dict)},
            "same_result_as_gls_run": t["same_result_as_gls_run"],
            "gap_pct": {k: None if v["mean_gap_pct"] is None else round(v["mean_gap_pct"], 3) for k, v in s["local_optimum"].items()}}
    for s in res["polish"]:
        if isinstance(s["cells"], list):
            brief[f"polish tsp{s['n']}x{s['instances']}"] = {
                str(c["budget_s"]): [round(c["mean_gap_before_pct"], 4), round(c["mean_gap_after_pct"], 4), round(c["share_moved"], 3),
                                     round(c["polish_s"], 4)] for c in s["cells"]}
    print(json.dumps(brief))
    return 0


if __name__ == "__main__":
    sys.exit(main())
