#!/usr/bin/env python
"""Measures iterated local search (ops.ils: ils_kernel in oropt_kernels.hip) against guided local search at equal device time, on
the instances bench.py searches, on one GPU.

    python scripts/bench_ils.py [--out profiles/ils.json] [--shapes 100x1024,200x256] [--kicks 0,10,100,1000] [--long_kicks 10000]

Per shape of --shapes (the leading instances of block 0 of the seeded test set: same generator and seed as bench.py), from the
nearest-neighbour start, at max_seg 3 with reversal:

1. device time -- HIP events on the stream, warm-up first, median of --repeats calls -- of ops.ils at every kick count of
   --kicks, the calls ALTERNATED inside every repeat, and the time per kick (the run's time less the kicks = 0 run's, per kick).
2. at every kick count: descent moves per kick, accepted kicks, runs the move cap ended, and the mean gap against the best-known
   lengths of bench_data/.
3. the equal-time comparison: the mean gap of solve_batch(guides=("weight",), budget="per_batch", time_limit=<that ILS run's
   median device time>) on the same instances.  ONE wall-clock run per cell: a cell carries the run-to-run spread of a wall-clock
   search, which this script does not measure.
4. the number of instances ILS ends more than 1e-9 (relative) BELOW the best-known length, with their indices: any such instance
   is a finding about bench_data/ (this script reports it and edits nothing).
5. --long_kicks K > 0: one run of K kicks as chained rounds of at most 1000 kicks (kick0 continues the kick counter, so the rounds
   ARE the one run), timed once with events around the rounds, with the same cells and its own equal-time search.

No threshold: the cells are recorded as measured.  "Guided search wins everywhere" is a result.
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

ROUND = 1000
BELOW = 1e-9


def gap_pct(cost, bk):
    return float(((cost / bk - 1) * 100).mean())


def quality(r, kicks, base_moves, bk):
    """The cells of one finished run (an IlsResult, or the sums of chained ones)."""
    cost = r["cost"]
    below = np.nonzero(cost < bk * (1 - BELOW))[0]
    return {"mean_length": float(cost.mean()), "mean_gap_pct": gap_pct(cost, bk),
            "moves_per_kick": None if kicks == 0 else float((r["moves"] - base_moves).mean() / kicks),
            "mean_accepted_kicks": float(r["accepted"].mean()), "move_cap": int(r["capped"]),
            "below_best_known": int(below.size), "below_best_known_instances": below.tolist(),
            "largest_relative_improvement": float((1 - cost[below] / bk[below]).max()) if below.size else 0.0}


def as_cells(r):
    return {"cost": r.cost.cpu().numpy(), "moves": r.moves.cpu().numpy().astype(np.int64), "accepted": r.accepted.cpu().numpy().astype(np.int64),
            "capped": int((r.status == ops.STATUS_MOVE_CAP).sum())}


def guided_at(D, bk, seconds):
    """The equal-time comparison: guided local search on the distances for the whole batch within `seconds`; one run."""
    r = pipeline.solve_batch(D, guides=("weight",), time_limit=seconds, budget="per_batch")
    return {"time_limit_s": seconds, "mean_gap_pct": gap_pct(r.best_cost.cpu().numpy(), bk), "search_s": r.timing["search_s"],
            "chunks": r.timing["chunks"], "mean_outer_iters": float(r.outer_iters.double().mean())}


def chained(init, cost, D, kicks, seed):
    """One run of `kicks` kicks as rounds of at most ROUND: -> (cells, device ms of the rounds together)."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    tour, c, moves, accepted, capped = init, cost, 0, 0, 0
    a.record()
    parts = []
    for k0 in range(0, kicks, ROUND):
        r = ops.ils_launch(tour, c, D, min(ROUND, kicks - k0), seed=seed, kick0=k0)
        tour, c = r.tour, r.cost
        parts.append(r)
    b.record()
    b.synchronize()
    for r in parts:
        moves = moves + r.moves.cpu().numpy().astype(np.int64)
        accepted = accepted + r.accepted.cpu().numpy().astype(np.int64)
        capped += int((r.status == ops.STATUS_MOVE_CAP).sum())
    return {"cost": c.cpu().numpy(), "moves": moves, "accepted": accepted, "capped": capped}, a.elapsed_time(b)


def measure(D, bk, kick_counts, long_kicks, seed, warmup, repeats):
    init = ops.nearest_neighbor(D)
    cost = ops.tour_cost(init, D)
    pipeline.solve_batch(D, guides=("weight",), time_limit=0.02, budget="per_batch")       # warm-up of the search path
    times = alternated_ms({f"kicks_{k}": (lambda k=k: ops.ils(init, cost, D, k, seed=seed)) for k in kick_counts}, warmup, repeats)
    base = times.get("kicks_0", {}).get("device_ms_median")
    base_moves = ops.or_opt_descent(init, cost, D).moves.cpu().numpy().astype(np.int64)
    out = {"nearest_neighbor_gap_pct": gap_pct(cost.cpu().numpy(), bk), "runs": []}
    for k in kick_counts:
        t = times[f"kicks_{k}"]
        row = {"kicks": k, **t, "ms_per_kick": None if (k == 0 or base is None) else (t["device_ms_median"] - base) / k,
               "ils": quality(as_cells(ops.ils(init, cost, D, k, seed=seed)), k, base_moves, bk),
               "guided_equal_time": guided_at(D, bk, t["device_ms_median"] / 1e3)}
        out["runs"].append(row)
    if long_kicks > 0:
        chained(init, cost, D, min(long_kicks, 2 * ROUND), seed)                            # warm-up
        cells, ms = chained(init, cost, D, long_kicks, seed)
        out["chained"] = {"kicks": long_kicks, "rounds": -(-long_kicks // ROUND), "device_ms_once": ms,
                          "ms_per_kick": None if base is None else (ms - base) / long_kicks,
                          "ils": quality(cells, long_kicks, base_moves, bk), "guided_equal_time": guided_at(D, bk, ms / 1e3)}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ils.json"))
    ap.add_argument("--shapes", default="100x1024,200x256", help="comma-separated n x instances")
    ap.add_argument("--kicks", default="0,10,100,1000", help="comma-separated kick counts of single launches")
    ap.add_argument("--long_kicks", type=int, default=10000, help="kicks of the chained run (rounds of 1000; 0 = none)")
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error("--repeats must be >= 5 (medians)")
    kick_counts = [int(k) for k in args.kicks.split(",") if k]
    res = {"command": f"python scripts/bench_ils.py --shapes {args.shapes} --kicks {args.kicks} --long_kicks {args.long_kicks} "
                      f"--seed {args.seed} --warmup {args.warmup} --repeats {args.repeats}", "device": torch.cuda.get_device_name(0),
           "seed": args.seed, "settings": "ops.ils(max_seg=3, reverse=True, default move cap), kick seed = --seed, nearest-neighbour start",
           "timing": f"HIP events on the stream, {args.warmup} warm-up calls, median of {args.repeats}, the calls alternated inside every "
                     "repeat; the chained run is timed once",
           "guided_equal_time": "solve_batch(guides=('weight',), budget='per_batch', time_limit=<the ILS run's device time>): ONE "
                                "wall-clock run per cell",
           "below_best_known": f"instances whose ILS length is more than {BELOW} (relative) below the best-known length of bench_data/",
           "shapes": []}
    for n, B in shapes_of(args.shapes):
        D = torch.from_numpy(instance_range(args.seed, n, 0, B)).cuda()
        bk, bk_how = load_best_known(None, n, args.seed, 0, B)
        if bk is None:
            res["shapes"].append({"n": n, "instances": B, "best_known": bk_how, "runs": "unmeasured"})
            continue
        res["shapes"].append({"n": n, "instances": B, "best_known": bk_how,
                              **measure(D, bk, kick_counts, args.long_kicks, args.seed, args.warmup, args.repeats)})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    brief = {}
    for s in res["shapes"]:
        if not isinstance(s["runs"], list):
            continue
        rows = s["runs"] + ([s["chained"]] if "chained" in s else [])
        brief[f"tsp{s['n']}x{s['instances']}"] = {
            str(r["kicks"]): {"ms": round(r.get("device_ms_median", r.get("device_ms_once")), 3),
                              "us_per_kick": None if r["ms_per_kick"] is None else round(1e3 * r["ms_per_kick"], 2),
                              "ils_gap_pct": round(r["ils"]["mean_gap_pct"], 4), "guided_gap_pct": round(r["guided_equal_time"]["mean_gap_pct"], 4),
                              "below_best_known": r["ils"]["below_best_known"]} for r in rows}
    print(json.dumps(brief))
    return 0


if __name__ == "__main__":
    sys.exit(main())
