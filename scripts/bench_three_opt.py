#!/usr/bin/env python
"""Measures the 3-opt scan and descent (ops.three_opt_best_move, ops.three_opt_descent; threeopt_kernels.hip) on the instances
bench.py searches, on one GPU.

    python scripts/bench_three_opt.py [--out profiles/three_opt.json] [--shapes 100x1024,200x256] [--after_shapes 100x1024,200x256]

Per shape of --shapes (the leading instances of block 0 of the seeded test set: same generator and seed as bench.py), from the
nearest-neighbour start:

1. device time -- HIP events on the stream, warm-up first, median of --repeats calls -- of ONE 3-opt scan
   (ops.three_opt_best_move), of ops.three_opt_descent and of ops.or_opt_descent(max_seg=3, reversal on) on the same load, the
   three calls ALTERNATED inside every repeat.
2. the local optimum's mean length against the best-known lengths of bench_data/, with the moves applied and the runs the move
   cap ended, for the 3-opt descent and for the Or-opt descent.

Per shape of --after_shapes: pipeline.solve_batch(guides=("weight",), budget="per_batch") at budgets of 0.1 / 0.3 / 1 s, then
ops.three_opt_descent(res.best_tour, res.best_cost, D): the share of instances the descent moved, the mean gap before and after,
and the descent's device time.  ONE wall-clock search per cell: a cell carries the run-to-run spread of a wall-clock search, which
this script does not measure.

The record names where D lived (`d_store`: the distance triangle in LDS up to ops.three_opt_lds_max_n() nodes, global memory beyond);
the other placement is measured by running this script on a library built with -DTHREEOPT_LDS_MAX_N=0 (GNNGLS_EXTRA_FLAGS at
build time, GNNGLS_HIP_SO at run time).

No threshold: the cells are recorded as measured.  A descent that finds nothing on converged tours is a result.
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

GRID_S = (0.1, 0.3, 1.0)


def gap_pct(cost, bk):
    return None if bk is None else float(((cost.cpu().numpy() / bk - 1) * 100).mean())


def d_store(n):
    return "lds_triangle" if n <= ops.three_opt_lds_max_n() else "global"


def measure_descent(D, bk, warmup, repeats):
    init = ops.nearest_neighbor(D)
    cost = ops.tour_cost(init, D)
    out = {"device_time": alternated_ms({
        "three_opt_scan": lambda: ops.three_opt_best_move(init, D),
        "or_opt_descent_seg3": lambda: ops.or_opt_descent(init, cost, D, 3, True),
        "three_opt_descent": lambda: ops.three_opt_descent(init, cost, D)}, warmup, repeats)}
    t = out["device_time"]
    t["three_opt_over_or_opt"] = t["three_opt_descent"]["device_ms_median"] / t["or_opt_descent_seg3"]["device_ms_median"]
    n = D.shape[1]
    t["scan_candidates"] = int(D.shape[0]) * 4 * (n * (n - 1) * (n - 2) // 6)
    t["scan_candidates_per_us"] = t["scan_candidates"] / (t["three_opt_scan"]["device_ms_median"] * 1e3)
    out["local_optimum"] = {"nearest_neighbor": {"mean_gap_pct": gap_pct(cost, bk)}}
    for name, r in (("three_opt", ops.three_opt_descent(init, cost, D)), ("or_opt_seg3", ops.or_opt_descent(init, cost, D, 3, True))):
        out["local_optimum"][name] = {"mean_length": float(r.cost.mean()), "mean_gap_pct": gap_pct(r.cost, bk),
                                      "mean_moves": float(r.moves.double().mean()),
                                      "move_cap": int((r.status == ops.STATUS_MOVE_CAP).sum())}
    return out


def measure_after_search(D, bk, warmup, repeats):
    pipeline.solve_batch(D, guides=("weight",), time_limit=0.05)       # warm-up: every kernel of the path has run once
    rows = []
    for s in GRID_S:
        res = pipeline.solve_batch(D, guides=("weight",), time_limit=s, perturbation_moves=20, budget="per_batch")
        tour, cost = res.best_tour.contiguous(), res.best_cost.contiguous()
        r = ops.three_opt_descent(tour, cost, D)
        ms = alternated_ms({"three_opt_descent": lambda: ops.three_opt_descent(tour, cost, D)}, warmup, repeats)["three_opt_descent"]
        rows.append({"budget_s": s, "mean_gap_before_pct": gap_pct(cost, bk), "mean_gap_after_pct": gap_pct(r.cost, bk),
                     "share_moved": float((r.moves > 0).double().mean()), "mean_gain": float((cost - r.cost).mean()),
                     "mean_moves": float(r.moves.double().mean()), "descent_ms": ms["device_ms_median"],
                     "descent_ms_all": ms["device_ms_all"], "search_s": res.timing["search_s"],
                     "mean_outer_iters": float(res.outer_iters.double().mean())})
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "three_opt.json"))
    ap.add_argument("--shapes", default="100x1024,200x256", help="scan and descent: comma-separated n x instances")
    ap.add_argument("--after_shapes", default="100x1024,200x256", help="3-opt after guided search: comma-separated n x instances")
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error("--repeats must be >= 5 (medians)")
    res = {"command": f"python scripts/bench_three_opt.py --shapes {args.shapes} --after_shapes {args.after_shapes} --seed {args.seed} "
                      f"--warmup {args.warmup} --repeats {args.repeats}", "device": torch.cuda.get_device_name(0), "seed": args.seed,
           "timing": f"HIP events on the stream, {args.warmup} warm-up calls, median of {args.repeats}, the calls alternated inside every repeat",
           "lds_max_n": ops.three_opt_lds_max_n(),
           "after_search_budget": "solve_batch(guides=('weight',), time_limit=s, budget='per_batch'), then ops.three_opt_descent on "
                                  "best_tour / best_cost, outside s; ONE wall-clock search per cell",
           "descent": [], "after_search": []}
    for n, B in shapes_of(args.shapes):
        D = torch.from_numpy(instance_range(args.seed, n, 0, B)).cuda()
        bk, bk_how = load_best_known(None, n, args.seed, 0, B)
        res["descent"].append({"n": n, "instances": B, "d_store": d_store(n), "best_known": bk_how,
                               **measure_descent(D, bk, args.warmup, args.repeats)})
    for n, B in shapes_of(args.after_shapes):
        D = torch.from_numpy(instance_range(args.seed, n, 0, B)).cuda()
        bk, bk_how = load_best_known(None, n, args.seed, 0, B)
        res["after_search"].append({"n": n, "instances": B, "d_store": d_store(n), "best_known": bk_how,
                                    "cells": measure_after_search(D, bk, args.warmup, args.repeats) if bk is not None else "unmeasured"})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    brief = {}
    for s in res["descent"]:
        t = s["device_time"]
        brief[f"descent tsp{s['n']}x{s['instances']} ({s['d_store']})"] = {
            "ms": {k: round(v["device_ms_median"], 3) for k, v in t.items() if isinstance(v, dict)},
            "gap_pct": {k: None if v["mean_gap_pct"] is None else round(v["mean_gap_pct"], 3) for k, v in s["local_optimum"].items()},
            "moves": {k: round(v["mean_moves"], 2) for k, v in s["local_optimum"].items() if "mean_moves" in v}}
    for s in res["after_search"]:
        if isinstance(s["cells"], list):
            brief[f"after search tsp{s['n']}x{s['instances']}"] = {
                str(c["budget_s"]): [round(c["mean_gap_before_pct"], 4), round(c["mean_gap_after_pct"], 4), round(c["share_moved"], 3),
                                     round(c["descent_ms"], 3)] for c in s["cells"]}
    print(json.dumps(brief))
    return 0


if __name__ == "__main__":
    sys.exit(main())
