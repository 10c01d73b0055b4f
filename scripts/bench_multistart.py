#!/usr/bin/env python
"""Measures the sampled start tours (ops.sample_nn_tours; reference algorithms.py:21-50) and the multi-start search built on
them (pipeline.solve_batch(starts=R)) on the instances bench.py searches.

    python scripts/bench_multistart.py [--out profiles/multistart.json] [--cells 100x16,100x64,200x16]

* device time of ops.sample_nn_tours for a device load of walks (TSP100 x 1,024 walks, TSP200 x 256 walks: one walk per
  instance, and the same number of walks on 16 instances): HIP events on the stream, warm-up first, median of --repeats calls;
* mean gap against the best-known lengths of bench_data/ for small batches (the leading instances of block 0 of the seeded test
  set), searched with the 'weight' guide for 0.1 / 0.3 / 1 s: starts = 1 against starts = R at the SAME budget in the same run.
  The budget is solve_batch's time_limit with budget="per_batch": start tours, the sampling launch and -- where instances x R
  exceeds the device capacity -- every round of the batch fit inside it, so a cell with more runs than search slots pays for them
  with shorter rounds.  No threshold: the cells are recorded as measured.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import instance_range, load_best_known  # noqa: E402
from gnngls_amd import ops, pipeline  # noqa: E402

GRID_S = (0.1, 0.3, 1.0)
STARTS = {100: (1, 4, 16, 64), 200: (1, 4, 16)}
WALK_SHAPES = ((100, 1024), (200, 256))


def device_ms(fn, warmup, repeats):
    """Median device milliseconds of fn() between two events on the current stream."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), [float(x) for x in ms]


def measure_sampler(n, walks, seed, warmup, repeats):
    out = {"n": n, "walks": walks, "layouts": {}}
    for B in (walks, 16):
        D = torch.from_numpy(instance_range(seed, n, 0, B)).cuda()
        R = walks // B
        med, raw = device_ms(lambda: ops.sample_nn_launch(D, R, 0, True, 1), warmup, repeats)
        nn, _ = device_ms(lambda: ops.nearest_neighbor(D), warmup, repeats)
        # bytes a launch requests from the memory system: one matrix row per step and walk (the rows come from L2 after the
        # first walk of an instance), the tour written once
        row_bytes = walks * (n - 1) * n * 8
        out["layouts"][f"{B}x{R}"] = {"instances": B, "walks_per_instance": R, "device_ms_median": med, "device_ms_all": raw,
                                      "nearest_neighbor_ms_same_instances": nn, "us_per_step": med * 1e3 / (n - 1),
                                      "row_bytes_requested": row_bytes, "row_gb_per_s": row_bytes / med / 1e6}
    return out


def measure_cell(n, B, seed):
    D = torch.from_numpy(instance_range(seed, n, 0, B)).cuda()
    bk, bk_how = load_best_known(None, n, seed, 0, B)
    out = {"n": n, "instances": B, "best_known": bk_how, "capacity": ops.gls_resident_capacity(n), "starts": {}}
    if bk is None:
        out["starts"] = "unmeasured"
        return out
    pipeline.solve_batch(D, guides=("weight",), time_limit=0.05, starts=2)       # warm-up: every kernel of the path has run once
    for R in STARTS[n]:
        row = {}
        for s in GRID_S:
            r = pipeline.solve_batch(D, guides=("weight",), time_limit=s, perturbation_moves=20, budget="per_batch", starts=R,
                                     start_seed=0)
            gap = (r.best_cost.cpu().numpy() / bk - 1.0) * 100.0
            cell = {"mean_gap_pct": float(gap.mean()), "max_gap_pct": float(gap.max()),
                    "at_best_known": int((np.abs(gap) <= 1e-9).sum()), "below_best_known": int((gap < -1e-9).sum()),
                    "chunks": r.timing["chunks"], "search_s": r.timing["search_s"], "init_s": r.timing["init_s"],
                    "sample_s": r.timing.get("sample_s", 0.0), "mean_outer_iters_of_winner": float(r.outer_iters.double().mean()),
                    "watchdog": int((r.status == ops.STATUS_WATCHDOG).sum())}
            if R > 1:
                cell["won_by_run_0"] = int((r.best_start == 0).sum())
                cell["run_0_mean_gap_pct"] = float(((r.start_costs[:, 0].cpu().numpy() / bk - 1.0) * 100.0).mean())
            row[str(s)] = cell
        out["starts"][str(R)] = row
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multistart.json"))
    ap.add_argument("--cells", default="100x16,100x64,200x16", help="comma-separated n x instances")
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error("--repeats must be >= 5 (medians)")
    res = {"command": f"python scripts/bench_multistart.py --cells {args.cells} --seed {args.seed} --warmup {args.warmup} "
                      f"--repeats {args.repeats}", "device": torch.cuda.get_device_name(0), "seed": args.seed,
           "timing": f"HIP events on the stream, {args.warmup} warm-up calls, median of {args.repeats}",
           "budget": "solve_batch(time_limit=s, budget='per_batch', guides=('weight',)): start tours, sampling and all rounds inside s",
           "sampler": [measure_sampler(n, walks, args.seed, args.warmup, args.repeats) for n, walks in WALK_SHAPES], "cells": []}
    for cell in args.cells.split(","):
        n, B = (int(x) for x in cell.split("x"))
        res["cells"].append(measure_cell(n, B, args.seed))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    brief = {f"tsp{c['n']}x{c['instances']}": {R: {s: round(v["mean_gap_pct"], 4) for s, v in row.items()}
                                               for R, row in c["starts"].items()} for c in res["cells"] if isinstance(c["starts"], dict)}
    print(json.dumps({"sampler_ms": {f"tsp{s['n']}": {k: round(v["device_ms_median"], 4) for k, v in s["layouts"].items()}
                                     for s in res["sampler"]}, "mean_gap_pct": brief}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
