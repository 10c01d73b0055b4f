#!/usr/bin/env python
"""Measures beam-search decoding (ops.beam_search: beam_search_kernel in beam_kernels.hip) -- its device time, the same steps as a
plain torch loop, and what a pure decode is worth against guided local search at equal device time -- on the instances bench.py
searches, on one GPU.

    python scripts/bench_beam.py [--out profiles/beam_search.json] [--shapes 100x1024,200x256] [--widths 1,16,128,1024]
                                 [--loop_widths 1,16,128,1024]

Per shape of --shapes (the leading instances of block 0 of the seeded test set: same generator and seed as bench.py):

1. device time -- HIP events on the stream, warm-up first, median of --repeats calls, the compared calls ALTERNATED inside every
   repeat -- per width of ops.beam_search(S = weight, select='score', no D) and, for the widths of --loop_widths, of
   torch_topk_loop below: the same steps in plain torch with one torch.topk over [B, width * n] per step.  Its tie order is
   undefined, so only the times are compared.
2. per width, for S from `weight`, from alpha-nearness and from the synthetic model's regret prediction, under select='score' and
   select='cost': ONE run timed with events, the mean gap of its best tours against the best-known lengths of bench_data/, and the
   same after ops.or_opt_descent on those tours (its device time apart).
3. the equal-time comparison, per width: the mean gap of solve_batch(guides=("weight",), budget="per_batch", time_limit=<the
   device time of the weight / select='cost' decode>) on the same instances.  ONE wall-clock run per cell.

No threshold: the cells are recorded as measured.  "The loop is as fast" and "guided search wins everywhere" are results.
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
from bench_aco import gap_pct, once_ms, score_stats  # noqa: E402
from bench_or_opt import alternated_ms, shapes_of  # noqa: E402
from gnngls_amd import ops, pipeline  # noqa: E402

ALPHA_ITERS = 100


def torch_topk_loop(S, width, depot=0):
    """The steps of ops.beam_search(select='score') as plumbing: per step one gather of the beams' rows, one add, one mask, one
    torch.topk over [B, beams * n], one gather / scatter of the visited bits; back-pointers walked once for the best beam.
    -> (best_tour [B,n+1] int64, best_score [B]).  torch.topk leaves the order of equal keys undefined."""
    B, n, _ = S.shape
    dev = S.device
    rows_of = torch.arange(B, device=dev)[:, None]
    c = torch.zeros((B, 1), dtype=torch.float64, device=dev)
    last = torch.full((B, 1), depot, dtype=torch.int64, device=dev)
    visited = torch.zeros((B, 1, n), dtype=torch.bool, device=dev)
    visited[:, :, depot] = True
    back = []
    for t in range(1, n):
        nb = c.shape[1]
        key = (c[:, :, None] + S[rows_of, last]).masked_fill_(visited, float("inf"))
        m = min(width, nb * (n - t))
        c, idx = torch.topk(key.view(B, nb * n), m, dim=1, largest=False, sorted=True)
        k, last = idx // n, idx % n
        visited = visited.gather(1, k[:, :, None].expand(B, m, n)).scatter_(2, last[:, :, None], True)
        back.append((k, last))
    score = c + S[rows_of, last, depot]
    best_score, r = score.min(dim=1, keepdim=True)
    tour = torch.full((B, n + 1), depot, dtype=torch.int64, device=dev)
    for t in range(n - 1, 0, -1):
        k, j = back[t - 1]
        tour[:, t] = j.gather(1, r)[:, 0]
        r = k.gather(1, r)
    return tour, best_score[:, 0]


def guides_of(D):
    """({name: S [B,n,n]}, {name: score_stats}) for the three edge scores the library has."""
    ub = ops.tour_cost(ops.nearest_neighbor(D), D)
    alpha = ops.alpha_nearness(D, ops.one_tree_bound(D, ub, max_iters=ALPHA_ITERS).pi)
    model = pipeline.synthetic_model(seed=1234)
    regret = pipeline.predict_regret(model, D, pipeline.Scalers.fit_weights(D)).to(torch.float64).contiguous()
    S = {"weight": D, "alpha": alpha.contiguous(), "regret_synthetic": regret}
    return S, {k: score_stats(v) for k, v in S.items()}


def measure(D, bk, widths, loop_widths, warmup, repeats):
    B, n, _ = D.shape
    S, scores = guides_of(D)
    init = ops.nearest_neighbor(D)
    init_cost = ops.tour_cost(init, D)
    nn_polished = ops.or_opt_descent(init, init_cost, D)                                   # also the warm-up of the descent
    pipeline.solve_batch(D, guides=("weight",), time_limit=0.02, budget="per_batch")       # ... and of the search path
    out = {"nearest_neighbor_gap_pct": gap_pct(init_cost.cpu().numpy(), bk),
           "nearest_neighbor_gap_pct_after_or_opt": gap_pct(nn_polished.cost.cpu().numpy(), bk),
           "guide_scores": scores, "device_time": [], "decode": []}
    for w in widths:
        ws = torch.empty(ops.beam_search_workspace_bytes(B, n, w), dtype=torch.uint8, device=D.device)
        fns = {"beam_search": lambda w=w, ws=ws: ops.beam_search(D, w, workspace=ws)}
        if w in loop_widths:
            fns["torch_topk_loop"] = lambda w=w: torch_topk_loop(D, w)
        t = alternated_ms(fns, warmup, repeats)
        row = {"width": w, "workspace_bytes": ws.numel(), **t}
        if w in loop_widths:
            row["loop_over_launch"] = t["torch_topk_loop"]["device_ms_median"] / t["beam_search"]["device_ms_median"]
            a, b = ops.beam_search(D, w), torch_topk_loop(D, w)
            row["same_best_score_instances"] = int((a.best_score == b[1]).sum())           # ties apart the two agree
        else:
            row["torch_topk_loop"] = "not run"
        out["device_time"].append(row)

        cell = {"width": w, "guides": {}}
        for name, G in S.items():
            cell["guides"][name] = {}
            for select in ("score", "cost"):
                try:
                    r, ms = once_ms(lambda: ops.beam_search(G, w, D=D, select=select, workspace=ws))
                except ValueError as e:                   # a score the decoder refuses: recorded, not hidden
                    cell["guides"][name][f"select_{select}"] = {"refused": str(e)[:200]}
                    continue
                d, dms = once_ms(lambda: ops.or_opt_descent(r.best_tour, r.best_cost, D))
                cell["guides"][name][f"select_{select}"] = {
                    "device_ms_once": ms, "mean_gap_pct": gap_pct(r.best_cost.cpu().numpy(), bk),
                    "or_opt_descent_ms_once": dms, "mean_gap_pct_after_or_opt": gap_pct(d.cost.cpu().numpy(), bk),
                    "or_opt_moves_mean": float(d.moves.double().mean())}
        seconds = cell["guides"]["weight"]["select_cost"]["device_ms_once"] / 1e3
        g = pipeline.solve_batch(D, guides=("weight",), time_limit=seconds, budget="per_batch")
        cell["guided_equal_time"] = {"time_limit_s": seconds, "mean_gap_pct": gap_pct(g.best_cost.cpu().numpy(), bk),
                                     "search_s": g.timing["search_s"], "chunks": g.timing["chunks"],
                                     "mean_outer_iters": float(g.outer_iters.double().mean())}
        out["decode"].append(cell)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "beam_search.json"))
    ap.add_argument("--shapes", default="100x1024,200x256", help="comma-separated n x instances")
    ap.add_argument("--widths", default="1,16,128,1024", help="comma-separated beam widths")
    ap.add_argument("--loop_widths", default="1,16,128,1024", help="the widths at which the torch loop is timed too ('' = none)")
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error("--repeats must be >= 5 (medians)")
    widths = [int(w) for w in args.widths.split(",") if w]
    loop_widths = {int(w) for w in args.loop_widths.split(",") if w}
    res = {"command": f"python scripts/bench_beam.py --shapes {args.shapes} --widths {args.widths} --loop_widths '{args.loop_widths}' "
                      f"--seed {args.seed} --warmup {args.warmup} --repeats {args.repeats}",
           "device": torch.cuda.get_device_name(0), "seed": args.seed,
           "settings": f"depot 0; alpha under the potentials of a {ALPHA_ITERS}-iteration ascent; regret from "
                       "pipeline.synthetic_model(seed=1234): the reference's architecture with seeded weights, it predicts nothing -- "
                       "where guide_scores shows it constant, its decode is decided by the tie rule (k, j) alone and is no model result",
           "timing": f"device_time: HIP events on the stream, {args.warmup} warm-up calls, median of {args.repeats}, beam_search "
                     "(S = weight, select='score', no D, workspace reused) and torch_topk_loop alternated inside every repeat; the "
                     "cells of `decode` are timed once",
           "guided_equal_time": "solve_batch(guides=('weight',), budget='per_batch', time_limit=<device time of the weight / "
                                "select='cost' decode>): ONE wall-clock run per cell",
           "shapes": []}
    for n, B in shapes_of(args.shapes):
        D = torch.from_numpy(instance_range(args.seed, n, 0, B)).cuda()
        bk, bk_how = load_best_known(None, n, args.seed, 0, B)
        if bk is None:
            res["shapes"].append({"n": n, "instances": B, "best_known": bk_how, "decode": "unmeasured"})
            continue
        res["shapes"].append({"n": n, "instances": B, "best_known": bk_how, **measure(D, bk, widths, loop_widths, args.warmup, args.repeats)})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    brief = {}
    for s in res["shapes"]:
        if not isinstance(s["decode"], list):
            continue
        cells = {}
        for t, c in zip(s["device_time"], s["decode"]):
            loop = t["torch_topk_loop"]
            cells[str(t["width"])] = {
                "ms": round(t["beam_search"]["device_ms_median"], 3),
                "loop_ms": round(loop["device_ms_median"], 3) if isinstance(loop, dict) else loop,
                **{g: {k: [round(v["mean_gap_pct"], 3), round(v["mean_gap_pct_after_or_opt"], 3)] if "mean_gap_pct" in v else "refused"
                       for k, v in sel.items()} for g, sel in c["guides"].items()},
                "guided_gap_pct": round(c["guided_equal_time"]["mean_gap_pct"], 3)}
        brief[f"tsp{s['n']}x{s['instances']}"] = {"nn_gap_pct": round(s["nearest_neighbor_gap_pct"], 3), **cells}
    print(json.dumps(brief))
    return 0


if __name__ == "__main__":
    sys.exit(main())
