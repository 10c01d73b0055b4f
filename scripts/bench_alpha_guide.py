#!/usr/bin/env python
"""Measures the alpha-nearness guide (ops.alpha_nearness, alpha_kernels.hip; pipeline.solve_batch(guides=("alpha", ...))) on the
instances bench.py searches, on one GPU.

    python scripts/bench_alpha_guide.py [--out profiles/alpha_guide.json] [--shapes 100x1024,200x256]

Per shape (the leading instances of block 0 of the seeded test set: same generator and seed as bench.py):

1. device time -- HIP events on the stream, warm-up first, median of --repeats calls -- of ops.one_tree_bound at max_iters
   100 / 500 / 2000 (ub = the nearest-neighbour tour's length, as solve_batch calls it), of ops.alpha_nearness under the
   potentials of the longest ascent, and of the regret forward (pipeline.predict_regret) of the same batch in the same run.  The
   forward runs the SYNTHETIC model (pipeline.synthetic_model: the reference's architecture with seeded weights): its time is the
   architecture's, its predictions guide nothing.  The one relation the code implies is recorded as a flag: alpha_nearness builds
   one spanning tree where the ascent builds up to 2000, so its device time has to be far below the bound's at max_iters = 2000.
2. mean gap against the best-known lengths of bench_data/ for the guides 'weight', 'alpha' and 'alpha weight' at budgets of
   0.1 / 0.3 / 1 s and alpha_iters 0 / 100 / 2000.  The budget is solve_batch's time_limit with budget="per_batch": the ascent,
   the alpha launch, the start tours and every round of the batch fit inside it.  ONE wall-clock run per cell: a cell carries the
   run-to-run spread of a wall-clock search, which this script does not measure.
3. the outer iterations per instance of every cell: alpha changes which edges are penalised, so the iteration rate may move.

No threshold: the cells are recorded as measured.
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
from bench_multistart import device_ms  # noqa: E402
from gnngls_amd import ops, pipeline  # noqa: E402

GRID_S = (0.1, 0.3, 1.0)
ASCENT_ITERS = (100, 500, 2000)
ALPHA_ITERS = (0, 100, 2000)
GUIDES = (("weight",), ("alpha",), ("alpha", "weight"))


def measure_device_time(D, warmup, repeats):
    n = D.shape[1]
    ub = ops.tour_cost(ops.nearest_neighbor(D), D)
    out = {"one_tree_bound": {}}
    for k in ASCENT_ITERS:
        med, raw = device_ms(lambda: ops.one_tree_bound(D, ub, max_iters=k), warmup, repeats)
        r = ops.one_tree_bound(D, ub, max_iters=k)
        out["one_tree_bound"][str(k)] = {"device_ms_median": med, "device_ms_all": raw, "mean_iters": float(r.iters.double().mean())}
    pi = r.pi
    med, raw = device_ms(lambda: ops.alpha_nearness(D, pi), warmup, repeats)
    zero, _ = device_ms(lambda: ops.alpha_nearness(D), warmup, repeats)
    A = ops.alpha_nearness(D, pi)
    iu = torch.triu_indices(n, n, 1, device=A.device)
    zeros = (A[:, iu[0], iu[1]] == 0).sum(dim=1).double()
    out["alpha_nearness"] = {"device_ms_median": med, "device_ms_all": raw, "device_ms_median_zero_pi": zero,
                             "mean_zero_pairs_per_instance": float(zeros.mean()), "symmetric": bool(torch.equal(A, A.transpose(1, 2))),
                             "min": float(A.min())}
    model = pipeline.synthetic_model(seed=1234)
    scalers = pipeline.Scalers.fit_weights(D)
    med, raw = device_ms(lambda: pipeline.predict_regret(model, D, scalers), warmup, repeats)
    out["regret_forward_synthetic_model"] = {"device_ms_median": med, "device_ms_all": raw}
    bound_ms = out["one_tree_bound"]["2000"]["device_ms_median"]
    out["alpha_over_bound_2000"] = out["alpha_nearness"]["device_ms_median"] / bound_ms
    out["alpha_far_below_bound_2000"] = bool(out["alpha_nearness"]["device_ms_median"] * 10 < bound_ms)
    return out


def measure_gaps(D, bk):
    pipeline.solve_batch(D, guides=("alpha", "weight"), time_limit=0.05, alpha_iters=10)     # warm-up: every kernel of the path has run once
    rows = []
    for guides in GUIDES:
        for k in (ALPHA_ITERS if "alpha" in guides else (None,)):
            for s in GRID_S:
                r = pipeline.solve_batch(D, guides=guides, time_limit=s, perturbation_moves=20, budget="per_batch",
                                         **({} if k is None else {"alpha_iters": k}))
                gap = (r.best_cost.cpu().numpy() / bk - 1.0) * 100.0
                rows.append({"guides": " ".join(guides), "alpha_iters": k, "budget_s": s, "mean_gap_pct": float(gap.mean()),
                             "max_gap_pct": float(gap.max()), "at_best_known": int((np.abs(gap) <= 1e-9).sum()),
                             "below_best_known": int((gap < -1e-9).sum()), "chunks": r.timing["chunks"],
                             "alpha_s": r.timing.get("alpha_s", 0.0), "init_s": r.timing["init_s"], "search_s": r.timing["search_s"],
                             "mean_outer_iters": float(r.outer_iters.double().mean()),
                             "outer_iters_per_search_s": float(r.outer_iters.double().mean()) / max(r.timing["search_s"], 1e-9),
                             "watchdog": int((r.status == ops.STATUS_WATCHDOG).sum())})
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "alpha_guide.json"))
    ap.add_argument("--shapes", default="100x1024,200x256", help="comma-separated n x instances")
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error("--repeats must be >= 5 (medians)")
    res = {"command": f"python scripts/bench_alpha_guide.py --shapes {args.shapes} --seed {args.seed} --warmup {args.warmup} "
                      f"--repeats {args.repeats}", "device": torch.cuda.get_device_name(0), "seed": args.seed,
           "timing": f"HIP events on the stream, {args.warmup} warm-up calls, median of {args.repeats}",
           "forward": "pipeline.predict_regret of pipeline.synthetic_model(seed=1234): the reference's architecture, seeded weights",
           "budget": "solve_batch(time_limit=s, budget='per_batch'): the ascent, the alpha launch, start tours and all rounds inside s; "
                     "ONE wall-clock run per cell",
           "shapes": []}
    for shape in args.shapes.split(","):
        n, B = (int(x) for x in shape.split("x"))
        D = torch.from_numpy(instance_range(args.seed, n, 0, B)).cuda()
        bk, bk_how = load_best_known(None, n, args.seed, 0, B)
        row = {"n": n, "instances": B, "best_known": bk_how, "capacity": ops.gls_resident_capacity(n),
               "device_time": measure_device_time(D, args.warmup, args.repeats)}
        row["cells"] = measure_gaps(D, bk) if bk is not None else "unmeasured"
        res["shapes"].append(row)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    brief = {}
    for s in res["shapes"]:
        t = s["device_time"]
        brief[f"tsp{s['n']}x{s['instances']}"] = {
            "bound_ms": {k: round(v["device_ms_median"], 3) for k, v in t["one_tree_bound"].items()},
            "alpha_ms": round(t["alpha_nearness"]["device_ms_median"], 3),
            "forward_ms": round(t["regret_forward_synthetic_model"]["device_ms_median"], 3),
            "alpha_far_below_bound_2000": t["alpha_far_below_bound_2000"],
            "mean_gap_pct": {f"{c['guides']}|{c['alpha_iters']}|{c['budget_s']}": round(c["mean_gap_pct"], 4) for c in s["cells"]}
            if isinstance(s["cells"], list) else "unmeasured"}
    print(json.dumps(brief))
    return 0


if __name__ == "__main__":
    sys.exit(main())
