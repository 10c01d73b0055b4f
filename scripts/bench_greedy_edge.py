#!/usr/bin/env python
"""Measures greedy edge matching (ops.greedy_edge: greedy_edge_kernel in greedy_edge_kernels.hip) -- its device time, its rounds,
the same decode as plumbing, and what the decoded tour is worth beside the other decoders and guided local search at equal device
time -- on the instances bench.py searches, on one GPU.

    python scripts/bench_greedy_edge.py [--out profiles/greedy_edge.json] [--shapes 100x1024,200x256,1000x4]

Per shape of --shapes (the leading instances of block 0 of the seeded test set: same generator and seed as bench.py):

1. device time -- HIP events on the stream, warm-up first, median of --repeats calls, the compared calls ALTERNATED inside every
   repeat -- of ops.greedy_edge_launch(S = weight, no D, no edges) and of argsort_keys below: the n (n - 1) / 2 keys of every
   instance gathered and sorted with one torch.argsort on the device.  That is only the first half of the decode as plumbing; the
   second, the sequential acceptance pass, runs on the host over the copied order and is timed once with the wall clock
   (host_acceptance_ms, the copy included).  The tours of the two are asserted equal first (instances with two equal keys are left
   out of that comparison: torch.argsort is not stable; uniform instances have none).
2. `rounds` per instance, mean and max, of the S = weight decode.
3. per guide -- `weight`, alpha-nearness and the synthetic model's regret prediction --: ONE decode timed with events, the mean gap
   of its tours against the best-known lengths of bench_data/, and the same after ops.or_opt_descent (its device time apart).
4. beside it: nearest neighbour, beam search of width 128 on `weight` (select='cost'), both also after or_opt_descent, and
   solve_batch(guides=("weight",), budget="per_batch", time_limit=<the device time of the weight decode>), and the same given the
   time of that decode and the descent behind it together: ONE wall-clock run each.

No threshold: the cells are recorded as measured.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from bench import instance_range, load_best_known  # noqa: E402
from bench_aco import gap_pct, once_ms  # noqa: E402
from bench_beam import guides_of  # noqa: E402
from bench_or_opt import alternated_ms, shapes_of  # noqa: E402
from gnngls_amd import ops, pipeline  # noqa: E402

BEAM_WIDTH = 128


def argsort_keys(S, iu, ju):
    """[B, n (n - 1) / 2] int64: per instance the order of its upper-triangle keys, one torch.argsort on the device."""
    return torch.argsort(S[:, iu, ju], dim=1)


def host_acceptance(order, iu, ju, n, depot=0):
    """The sequential half of the decode on the host: the edges in `order`, accepted while both ends have degree below 2 and they are
    not the two ends of one fragment; then the closing edge and the tour from the depot towards its smaller neighbour."""
    tours = np.empty((order.shape[0], n + 1), dtype=np.int32)
    for b, o in enumerate(order):
        deg, other, nbr, left = [0] * n, list(range(n)), [[] for _ in range(n)], n - 1
        for i, j in zip(iu[o].tolist(), ju[o].tolist()):
            if deg[i] < 2 and deg[j] < 2 and other[i] != j:
                a, c = other[i], other[j]
                other[a], other[c] = c, a
                deg[i] += 1
                deg[j] += 1
                nbr[i].append(j)
                nbr[j].append(i)
                left -= 1
                if left == 0:
                    break
        e0, e1 = (u for u in range(n) if deg[u] == 1)
        nbr[e0].append(e1)
        nbr[e1].append(e0)
        prev, cur = depot, min(nbr[depot])
        tours[b, 0] = tours[b, n] = depot
        for q in range(1, n):
            tours[b, q] = cur
            x, y = nbr[cur]
            prev, cur = cur, (y if x == prev else x)
    return tours


def measure_time(D, warmup, repeats):
    """The device time, the plumbing and the rounds: needs no best-known lengths, so every shape has these cells."""
    B, n, _ = D.shape
    iu, ju = torch.triu_indices(n, n, 1, device=D.device)
    iu_h, ju_h = iu.cpu().numpy(), ju.cpu().numpy()

    # the plumbing decodes the same tours (tie-free instances), or the script stops
    mine = ops.greedy_edge(D)
    t0 = time.perf_counter()
    order = argsort_keys(D, iu, ju).cpu().numpy()
    t1 = time.perf_counter()
    theirs = host_acceptance(order, iu_h, ju_h, n)
    host_ms = (time.perf_counter() - t1) * 1e3
    keys = np.sort(D[:, iu, ju].cpu().numpy(), axis=1)
    tie_free = (np.diff(keys, axis=1) != 0).all(axis=1)
    assert np.array_equal(mine.tour.cpu().numpy()[tie_free], theirs[tie_free]), "greedy_edge and the argsort decode returned different tours"

    t = alternated_ms({"greedy_edge": lambda: ops.greedy_edge_launch(D), "argsort_keys_device": lambda: argsort_keys(D, iu, ju)},
                      warmup, repeats)
    t["host_acceptance_ms"] = host_ms
    t["argsort_copy_wall_ms"] = (t1 - t0) * 1e3
    t["same_tours_as_argsort"] = True
    t["tie_free_instances"] = int(tie_free.sum())
    t["argsort_over_launch"] = t["argsort_keys_device"]["device_ms_median"] / t["greedy_edge"]["device_ms_median"]
    rounds = mine.rounds.double()
    return {"device_time": t, "rounds": {"mean": float(rounds.mean()), "max": int(rounds.max())}}


def measure_quality(D, bk, seconds):
    """The gaps of the decoded tours beside the other decoders' and guided search within `seconds` of device time."""
    S, scores = guides_of(D)
    init = ops.nearest_neighbor(D)
    init_cost = ops.tour_cost(init, D)
    nn_polished = ops.or_opt_descent(init, init_cost, D)                                   # also the warm-up of the descent
    pipeline.solve_batch(D, guides=("weight",), time_limit=0.02, budget="per_batch")       # ... and of the search path
    beam = ops.beam_search(D, BEAM_WIDTH, D=D, select="cost")
    beam_polished = ops.or_opt_descent(beam.best_tour, beam.best_cost, D)
    out = {"guide_scores": scores,
           "nearest_neighbor_gap_pct": gap_pct(init_cost.cpu().numpy(), bk),
           "nearest_neighbor_gap_pct_after_or_opt": gap_pct(nn_polished.cost.cpu().numpy(), bk),
           f"beam_{BEAM_WIDTH}_weight_gap_pct": gap_pct(beam.best_cost.cpu().numpy(), bk),
           f"beam_{BEAM_WIDTH}_weight_gap_pct_after_or_opt": gap_pct(beam_polished.cost.cpu().numpy(), bk), "decode": {}}
    for name, G in S.items():
        G = torch.triu(G, 1)
        G = (G + G.transpose(1, 2)).contiguous()          # the key of {i, j} is the upper triangle's; the kernel reads rows
        r, ms = once_ms(lambda: ops.greedy_edge_launch(G, D=D))
        if r.status.any():                                # a score the decoder refuses: recorded, not hidden
            out["decode"][name] = {"refused": f"status {sorted(set(r.status.tolist()))}"}
            continue
        d, dms = once_ms(lambda: ops.or_opt_descent(r.tour, r.cost, D))
        out["decode"][name] = {"device_ms_once": ms, "mean_gap_pct": gap_pct(r.cost.cpu().numpy(), bk),
                               "rounds_mean": float(r.rounds.double().mean()), "rounds_max": int(r.rounds.max()),
                               "or_opt_descent_ms_once": dms, "mean_gap_pct_after_or_opt": gap_pct(d.cost.cpu().numpy(), bk),
                               "or_opt_moves_mean": float(d.moves.double().mean())}
    w = out["decode"]["weight"]
    for key, limit in (("guided_equal_time", seconds),
                       ("guided_equal_time_with_descent", (w["device_ms_once"] + w["or_opt_descent_ms_once"]) / 1e3 if "device_ms_once" in w else None)):
        if limit is None:
            continue
        g = pipeline.solve_batch(D, guides=("weight",), time_limit=limit, budget="per_batch")
        out[key] = {"time_limit_s": limit, "mean_gap_pct": gap_pct(g.best_cost.cpu().numpy(), bk), "search_s": g.timing["search_s"],
                    "chunks": g.timing["chunks"], "mean_outer_iters": float(g.outer_iters.double().mean())}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "greedy_edge.json"))
    ap.add_argument("--shapes", default="100x1024,200x256,1000x4", help="comma-separated n x instances")
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error("--repeats must be >= 5 (medians)")
    res = {"command": f"python scripts/bench_greedy_edge.py --shapes {args.shapes} --seed {args.seed} --warmup {args.warmup} "
                      f"--repeats {args.repeats}",
           "device": torch.cuda.get_device_name(0), "seed": args.seed,
           "settings": "depot 0; alpha under the potentials of a 100-iteration ascent; regret from pipeline.synthetic_model(seed=1234): "
                       "the reference's architecture with seeded weights, it predicts nothing -- where guide_scores shows it constant, "
                       "its decode is decided by the tie rule (i, j) alone and is no model result",
           "timing": f"device_time: HIP events on the stream, {args.warmup} warm-up calls, median of {args.repeats}, greedy_edge_launch "
                     "(S = weight, no D, no edges) and argsort_keys_device (torch.argsort over [B, n(n-1)/2] keys) alternated inside "
                     "every repeat; host_acceptance_ms is ONE wall-clock run of the sequential pass in Python over the copied order; "
                     "the cells of `decode` are timed once",
           "guided_equal_time": "solve_batch(guides=('weight',), budget='per_batch', time_limit=<median device time of the weight "
                                "decode>), guided_equal_time_with_descent: <the once-timed weight decode + its or_opt_descent>; ONE "
                                "wall-clock run each per shape",
           "shapes": []}
    for n, B in shapes_of(args.shapes):
        D = torch.from_numpy(instance_range(args.seed, n, 0, B)).cuda()
        bk, bk_how = load_best_known(None, n, args.seed, 0, B)
        cell = {"n": n, "instances": B, "best_known": bk_how, **measure_time(D, args.warmup, args.repeats)}
        if bk is None:                                    # no lengths to compare with (and beyond the regret model's n): times only
            cell["decode"] = "unmeasured"
        else:
            cell.update(measure_quality(D, bk, cell["device_time"]["greedy_edge"]["device_ms_median"] / 1e3))
        res["shapes"].append(cell)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    brief = {}
    for s in res["shapes"]:
        cells = {"ms": round(s["device_time"]["greedy_edge"]["device_ms_median"], 3),
                 "argsort_ms": round(s["device_time"]["argsort_keys_device"]["device_ms_median"], 3),
                 "host_pass_ms": round(s["device_time"]["host_acceptance_ms"], 1), "rounds": s["rounds"]}
        brief[f"tsp{s['n']}x{s['instances']}"] = cells
        if not isinstance(s["decode"], dict):
            continue
        cells.update({
            "nn_gap_pct": round(s["nearest_neighbor_gap_pct"], 3),
            **{g: ([round(c["mean_gap_pct"], 3), round(c["mean_gap_pct_after_or_opt"], 3)] if "mean_gap_pct" in c else "refused")
               for g, c in s["decode"].items()},
            "guided_gap_pct": round(s["guided_equal_time"]["mean_gap_pct"], 3),
            "guided_with_descent_gap_pct": round(s["guided_equal_time_with_descent"]["mean_gap_pct"], 3)})
    print(json.dumps(brief))
    return 0


if __name__ == "__main__":
    sys.exit(main())
