#!/usr/bin/env python
"""Measures the MAX-MIN ant system (ops.aco: aco_kernel in aco_kernels.hip) -- its device time per iteration and what it is worth
against guided local search at equal device time -- on the instances bench.py searches, on one GPU.

    python scripts/bench_aco.py [--out profiles/aco.json] [--shapes 100x1024,200x256] [--ants 16] [--iters 10,100,1000]
                                [--time_shapes 200x16x64]

Per shape of --shapes (the leading instances of block 0 of the seeded test set: same generator and seed as bench.py), with
--ants ants, rho 0.1, min_ratio 1 / (2 n), gb_every 0, spread starts, tau from the nearest-neighbour tour:

1. device time -- HIP events on the stream, warm-up first, median of --repeats calls, the calls ALTERNATED inside every repeat --
   of ops.aco on H = weight ** -2 at the two smallest iteration counts of --iters, and the time per iteration (their difference
   over the difference of the counts).  --time_shapes n x instances x ants adds shapes that are timed only.
2. at every iteration count of --iters, for H from `weight` (inverse, beta 2), from alpha-nearness and from the synthetic model's
   regret prediction (both shifted, beta 2): ONE run timed with events, the mean gap of its best tours against the best-known
   lengths of bench_data/, the same after ops.or_opt_descent on those tours (its device time apart), and how many instances ended
   below the best-known length.
3. the equal-time comparison, per iteration count: the mean gap of solve_batch(guides=("weight",), budget="per_batch",
   time_limit=<the weight run's device time>) on the same instances.  ONE wall-clock run per cell.

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

RHO = 0.1
BELOW = 1e-9
ALPHA_ITERS = 100


def gap_pct(cost, bk):
    return float(((cost / bk - 1) * 100).mean())


def once_ms(fn):
    """-> (fn's result, device ms of the one call)."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = fn()
    b.record()
    b.synchronize()
    return r, a.elapsed_time(b)


def score_stats(G):
    """Off-diagonal min / mean / max of an edge score over the batch (a constant score has no shifted heuristic: 0 / 0)."""
    g = G[:, ~torch.eye(G.shape[1], dtype=torch.bool, device=G.device)]
    return {"min": float(g.min()), "mean": float(g.mean()), "max": float(g.max()),
            "constant_instances": int((g.amax(dim=1) == g.amin(dim=1)).sum())}


def heuristics(D):
    """({name: H [B,n,n]}, {name: score_stats of the edge score behind it}) for the three guides the library has."""
    ub = ops.tour_cost(ops.nearest_neighbor(D), D)
    alpha = ops.alpha_nearness(D, ops.one_tree_bound(D, ub, max_iters=ALPHA_ITERS).pi)
    model = pipeline.synthetic_model(seed=1234)
    regret = pipeline.predict_regret(model, D, pipeline.Scalers.fit_weights(D)).to(torch.float64)
    return ({"weight_inverse": ops.aco_heuristic(D, 2.0, "inverse"), "alpha_shifted": ops.aco_heuristic(alpha, 2.0, "shifted"),
             "regret_synthetic_shifted": ops.aco_heuristic(regret, 2.0, "shifted")},
            {"weight_inverse": score_stats(D), "alpha_shifted": score_stats(alpha), "regret_synthetic_shifted": score_stats(regret)})


def time_per_iteration(D, H, ants, counts, seed, warmup, repeats):
    tau0 = ops.aco_init_tau(D, RHO)
    lo, hi = counts
    t = alternated_ms({f"iters_{k}": (lambda k=k: ops.aco(D, H, ants=ants, iters=k, rho=RHO, seed=seed, tau=tau0.clone())) for k in (lo, hi)},
                      warmup, repeats)
    return {**t, "ms_per_iteration": (t[f"iters_{hi}"]["device_ms_median"] - t[f"iters_{lo}"]["device_ms_median"]) / (hi - lo)}


def measure(D, bk, ants, iter_counts, seed, warmup, repeats):
    Hs, scores = heuristics(D)
    tau0 = ops.aco_init_tau(D, RHO)
    init = ops.nearest_neighbor(D)
    out = {"nearest_neighbor_gap_pct": gap_pct(ops.tour_cost(init, D).cpu().numpy(), bk), "ants": ants, "guide_scores": scores,
           "device_time": time_per_iteration(D, Hs["weight_inverse"], ants, sorted(iter_counts)[:2], seed, warmup, repeats), "runs": []}
    pipeline.solve_batch(D, guides=("weight",), time_limit=0.02, budget="per_batch")       # warm-up of the search path
    ops.or_opt_descent(init, ops.tour_cost(init, D), D)                                    # ... and of the descent
    for k in iter_counts:
        row = {"iters": k, "guides": {}}
        for name, H in Hs.items():
            try:
                r, ms = once_ms(lambda: ops.aco(D, H, ants=ants, iters=k, rho=RHO, seed=seed, tau=tau0.clone(), want_trace=True))
            except ValueError as e:                       # a guide whose H is no set of weights: recorded, not hidden
                row["guides"][name] = {"bad_weights": str(e)[:200]}
                continue
            d, dms = once_ms(lambda: ops.or_opt_descent(r.best_tour, r.best_cost, D))
            cost, dcost = r.best_cost.cpu().numpy(), d.cost.cpu().numpy()
            first = r.trace_cost[:, 0].cpu().numpy()
            row["guides"][name] = {"device_ms_once": ms, "mean_gap_pct": gap_pct(cost, bk), "first_iteration_gap_pct": gap_pct(first, bk),
                                   "or_opt_descent_ms_once": dms, "mean_gap_pct_after_or_opt": gap_pct(dcost, bk),
                                   "or_opt_moves_mean": float(d.moves.double().mean()),
                                   "below_best_known": int((cost < bk * (1 - BELOW)).sum()),
                                   "below_best_known_after_or_opt": int((dcost < bk * (1 - BELOW)).sum())}
        seconds = row["guides"]["weight_inverse"]["device_ms_once"] / 1e3
        g = pipeline.solve_batch(D, guides=("weight",), time_limit=seconds, budget="per_batch")
        row["guided_equal_time"] = {"time_limit_s": seconds, "mean_gap_pct": gap_pct(g.best_cost.cpu().numpy(), bk),
                                    "search_s": g.timing["search_s"], "chunks": g.timing["chunks"],
                                    "mean_outer_iters": float(g.outer_iters.double().mean())}
        out["runs"].append(row)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aco.json"))
    ap.add_argument("--shapes", default="100x1024,200x256", help="comma-separated n x instances")
    ap.add_argument("--ants", type=int, default=16)
    ap.add_argument("--iters", default="10,100,1000", help="comma-separated iteration counts (at least two)")
    ap.add_argument("--time_shapes", default="200x16x64", help="timed only: comma-separated n x instances x ants ('' = none)")
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error("--repeats must be >= 5 (medians)")
    iter_counts = [int(k) for k in args.iters.split(",") if k]
    if len(set(iter_counts)) < 2:
        ap.error("--iters needs two different counts (the time per iteration is a difference)")
    res = {"command": f"python scripts/bench_aco.py --shapes {args.shapes} --ants {args.ants} --iters {args.iters} --time_shapes "
                      f"'{args.time_shapes}' --seed {args.seed} --warmup {args.warmup} --repeats {args.repeats}",
           "device": torch.cuda.get_device_name(0), "seed": args.seed,
           "settings": f"ops.aco(rho={RHO}, min_ratio=1/(2n), gb_every=0, spread_starts=True, tau from the nearest-neighbour tour), Philox "
                       f"seed = --seed; alpha under the potentials of a {ALPHA_ITERS}-iteration ascent; regret from "
                       "pipeline.synthetic_model(seed=1234): the reference's architecture with seeded weights, it predicts nothing",
           "timing": f"device_time: HIP events on the stream, {args.warmup} warm-up calls, median of {args.repeats}, the calls alternated "
                     "inside every repeat; the cells of `runs` are timed once",
           "guided_equal_time": "solve_batch(guides=('weight',), budget='per_batch', time_limit=<the weight run's device time>): ONE "
                                "wall-clock run per cell",
           "below_best_known": f"instances more than {BELOW} (relative) below the best-known length of bench_data/",
           "shapes": [], "time_only": []}
    for n, B in shapes_of(args.shapes):
        D = torch.from_numpy(instance_range(args.seed, n, 0, B)).cuda()
        bk, bk_how = load_best_known(None, n, args.seed, 0, B)
        if bk is None:
            res["shapes"].append({"n": n, "instances": B, "best_known": bk_how, "runs": "unmeasured"})
            continue
        res["shapes"].append({"n": n, "instances": B, "best_known": bk_how,
                              **measure(D, bk, args.ants, iter_counts, args.seed, args.warmup, args.repeats)})
    for n, B, R in shapes_of(args.time_shapes):
        D = torch.from_numpy(instance_range(args.seed, n, 0, B)).cuda()
        res["time_only"].append({"n": n, "instances": B, "ants": R,
                                 **time_per_iteration(D, ops.aco_heuristic(D, 2.0, "inverse"), R, sorted(iter_counts)[:2], args.seed,
                                                      args.warmup, args.repeats)})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    brief = {}
    for s in res["shapes"]:
        if not isinstance(s["runs"], list):
            continue
        brief[f"tsp{s['n']}x{s['instances']}"] = {
            "ms_per_iteration": round(s["device_time"]["ms_per_iteration"], 4),
            **{str(r["iters"]): {"ms": round(r["guides"]["weight_inverse"]["device_ms_once"], 2),
                                 **{g: [round(c["mean_gap_pct"], 3), round(c["mean_gap_pct_after_or_opt"], 3)] if "mean_gap_pct" in c
                                    else "bad_weights" for g, c in r["guides"].items()},
                                 "guided_gap_pct": round(r["guided_equal_time"]["mean_gap_pct"], 3)} for r in s["runs"]}}
    for s in res["time_only"]:
        brief[f"tsp{s['n']}x{s['instances']}_ants{s['ants']}"] = {"ms_per_iteration": round(s["ms_per_iteration"], 4)}
    print(json.dumps(brief))
    return 0


if __name__ == "__main__":
    sys.exit(main())
