#!/usr/bin/env python
"""Measures the insertion tour constructors (ops.insertion; reference algorithms.py:82-108) on the instances bench.py searches.

    python scripts/bench_constructors.py [--out profiles/insertion_constructors.json] [--shapes 100x1024,200x256]

Per shape (the leading instances of block 0 of the seeded test set: same generator and seed as bench.py, so the best-known
lengths of bench_data/ apply):

* device time of ops.nearest_neighbor, ops.insertion nearest / farthest (on the distances and on the model's regret_pred
  matrix) and of the regret forward of the same batch, in the same run: HIP events on the stream, warm-up first, median of
  --repeats timed calls.  THE ONE CONDITION (exit status 1 if it fails): every insertion of a device load takes less than the
  forward pass of that load.
* mean start-tour length over the best-known length, nearest neighbour against both insertions;
* mean gap after 0.1 / 0.3 / 1 s of SEARCH (solve_batch, budget="per_instance"; read from the improvement record like
  bench.py's gap_vs_budget) for each start: 'weight' guide, and 'regret_pred' guide with init_weight "auto" and "weight".
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import best_at_times, instance_range, load_best_known  # noqa: E402
from gnngls_amd import models as M  # noqa: E402
from gnngls_amd import ops, pipeline  # noqa: E402

GRID_S = (0.1, 0.3, 1.0)
STARTS = ("nearest_neighbor", "nearest_insertion", "farthest_insertion")
IMP_CAP = 256


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


def start_tour(W, start):
    return ops.nearest_neighbor(W) if start == "nearest_neighbor" else ops.insertion(W, 0, pipeline.INIT_TOURS[start])


def measure_shape(n, B, seed, model, warmup, repeats, skip_search):
    D = torch.from_numpy(instance_range(seed, n, 0, B)).cuda()
    bk, bk_how = load_best_known(None, n, seed, 0, B)
    scalers = pipeline.Scalers.fit_weights(torch.from_numpy(instance_range(seed, n, 0, 1024)).cuda())
    feat = M.pack_features(D, scalers.feat_scale, scalers.feat_min)
    R = pipeline.predict_regret(model, D, scalers)
    out = {"n": n, "instances": B, "best_known": bk_how}

    t = {}
    t["regret_forward_ms"], raw_fwd = device_ms(lambda: M.regret_forward(model, feat, B, n), warmup, repeats)
    t["predict_regret_ms"], _ = device_ms(lambda: pipeline.predict_regret(model, D, scalers), warmup, repeats)   # + pack / unpack
    t["nearest_neighbor_ms"], _ = device_ms(lambda: ops.nearest_neighbor(D), warmup, repeats)
    raw = {"regret_forward_ms": raw_fwd}
    for name, W in (("weight", D), ("regret_pred", R)):
        for mode in ("nearest", "farthest"):
            key = f"insertion_{mode}_on_{name}_ms"
            t[key], raw[key] = device_ms(lambda: ops.insertion(W, 0, mode), warmup, repeats)
    out["device_time_ms_median"] = t
    out["device_time_ms_all"] = raw
    slowest = max(v for k, v in t.items() if k.startswith("insertion_"))
    out["slowest_insertion_over_forward"] = slowest / t["regret_forward_ms"]
    out["insertion_faster_than_forward"] = bool(slowest < t["regret_forward_ms"])

    lengths = {}
    for start in STARTS:
        c = ops.tour_cost(start_tour(D, start), D).cpu().numpy()
        lengths[start] = {"mean_length": float(c.mean()),
                          "mean_over_best_known_pct": float(((c / bk - 1.0) * 100.0).mean()) if bk is not None else "unmeasured"}
    out["start_tour_on_weight"] = lengths

    if skip_search or bk is None:
        out["gap_after_search"] = "unmeasured"
        return out
    configs = (("weight", ("weight",), "auto"), ("regret_pred,init_weight=auto", ("regret_pred",), "auto"),
               ("regret_pred,init_weight=weight", ("regret_pred",), "weight"))
    gaps = {}
    for label, guides, init_weight in configs:
        need = "regret_pred" in guides
        pre = 2.0 * t["predict_regret_ms"] / 1e3 + 0.2 if need else 0.2          # the budget clock starts before the forward pass
        row = {}
        for start in STARTS:
            r = pipeline.solve_batch(D, model if need else None, scalers if need else None, guides=guides,
                                     time_limit=GRID_S[-1] + pre, perturbation_moves=20, budget="per_instance", imp_cap=IMP_CAP,
                                     init=start, init_weight=init_weight)
            imp_len = r.imp_len.cpu().numpy()
            imp_time = r.imp_time.cpu().numpy()
            best_t, truncated = best_at_times(r.imp_cost.cpu().numpy(), imp_time, imp_len, r.init_cost.cpu().numpy(), GRID_S)
            end = imp_time[np.arange(B), np.minimum(imp_len, IMP_CAP) - 1]        # the terminal entry: end of the search
            g = (best_t / bk[:, None] - 1.0) * 100.0
            row[start] = {"init_mean_gap_pct": float(((r.init_cost.cpu().numpy() / bk - 1.0) * 100.0).mean()),
                          "mean_gap_pct_after_search_s": {str(s): float(g[:, k].mean()) for k, s in enumerate(GRID_S)},
                          "search_s_min": float(end.min()), "chunks": r.timing["chunks"],
                          "truncated_records": int(truncated.sum()), "watchdog": int((r.status == ops.STATUS_WATCHDOG).sum())}
        gaps[label] = row
    out["gap_after_search"] = gaps
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "insertion_constructors.json"))
    ap.add_argument("--shapes", default="100x1024,200x256", help="comma-separated n x instances")
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--skip_search", action="store_true", help="timings and start-tour lengths only")
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error("--repeats must be >= 5 (medians)")
    model = pipeline.synthetic_model(seed=1234)
    res = {"command": f"python scripts/bench_constructors.py --shapes {args.shapes} --seed {args.seed} --warmup {args.warmup} "
                      f"--repeats {args.repeats}" + (" --skip_search" if args.skip_search else ""), "device": torch.cuda.get_device_name(0),
           "seed": args.seed, "model": "pipeline.synthetic_model(seed=1234): the reference architecture, synthetic weights (as bench.py)",
           "timing": f"HIP events on the stream, {args.warmup} warm-up calls, median of {args.repeats}", "shapes": []}
    for shape in args.shapes.split(","):
        n, B = (int(x) for x in shape.split("x"))
        res["shapes"].append(measure_shape(n, B, args.seed, model, args.warmup, args.repeats, args.skip_search))
    res["condition"] = "every insertion of a device load takes less device time than the regret forward of that load"
    res["condition_holds"] = all(s["insertion_faster_than_forward"] for s in res["shapes"])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({"condition_holds": res["condition_holds"],
                      "shapes": [{"n": s["n"], "instances": s["instances"], **s["device_time_ms_median"]} for s in res["shapes"]]}))
    return 0 if res["condition_holds"] else 1


if __name__ == "__main__":
    sys.exit(main())
