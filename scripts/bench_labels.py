#!/usr/bin/env python
"""Throughput of regret-label generation on one MI355X: prints one JSON line.

    python scripts/bench_labels.py [--sizes 20,50,100] [--rocprof]

Per size: fixed-edge searches per second and instances per second of one labelling round (gnngls_regret_labels over every
edge off the base tour, at the default budget: labels.LABEL_ITERS outer iterations, labels.PERTURBATION_MOVES), base tours
prepared beforehand (labels.base_tours, not timed); and the CPU baseline, the oracle (oracle/gls_oracle.c, the same search)
on one core on a sample of the same jobs.  With --rocprof the same workload runs once more under
`rocprofv3 --kernel-trace --stats` in a child process, and the kernel time is split into expansion (label_expand + the
start-tour cost), search (the persistent search kernel and its set-up kernels) and labelling (label_cost / label_best /
label_finalize and the per-instance offsets).
"""
import argparse
import csv
import glob
import itertools
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BATCH = {20: 512, 50: 64, 100: 16}


def gpu_rates(sizes, repeat):
    import torch

    from gnngls_amd import labels
    from gnngls_amd.synthetic import random_instances
    out = {}
    for n in sizes:
        B = BATCH.get(n, max(1, 40000 // (n * (n - 1) // 2 - n)))
        D, _ = random_instances(np.random.default_rng(2024 + n), B, n)
        Dd = torch.from_numpy(D).cuda()
        base = labels.base_tours(Dd)
        labels.fixed_edge_labels(Dd[:1].contiguous(), base[:1].contiguous())          # warm-up (library, allocator)
        torch.cuda.synchronize()
        best = None
        for _ in range(repeat):
            t0 = time.perf_counter()
            _, _, _, _, st = labels.fixed_edge_labels(Dd, base)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        assert not bool((st == labels.STATUS_EDGE_LOST).any())
        jobs = B * (n * (n - 1) // 2 - n)
        out[n] = dict(instances=B, jobs=jobs, seconds=best, searches_per_s=jobs / best, instances_per_s=B / best,
                      chunk_jobs=labels._lib.load().gnngls_regret_labels_chunk(n))
    return out


def cpu_rate(n, jobs=6):
    from gnngls_amd import labels
    from gnngls_amd.synthetic import random_instances
    from oracle import gls_oracle as go
    D, _ = random_instances(np.random.default_rng(2024 + n), 1, n)
    base = go.guided_local_search(D[0], D[0][None], go.nearest_neighbor(D[0]), go.tour_cost(go.nearest_neighbor(D[0]), D[0]),
                                  perturbation_moves=labels.PERTURBATION_MOVES, max_outer_iters=labels.SOLVE_ITERS,
                                  want_penalty=False, trace_cap=1)["best_tour"]
    on = {frozenset((base[p], base[p + 1])) for p in range(n)}
    off = [e for e in itertools.combinations(range(n), 2) if frozenset(e) not in on]
    pick = [off[q] for q in np.random.default_rng(n).choice(len(off), jobs, replace=False)]
    t0 = time.perf_counter()
    for i, j in pick:
        Dp = labels.fixed_edge_matrix(D[0], i, j)
        go.guided_local_search(Dp, Dp[None], np.array(base, dtype=np.int32), go.tour_cost(base, Dp),
                               perturbation_moves=labels.PERTURBATION_MOVES, max_outer_iters=labels.LABEL_ITERS,
                               want_penalty=False, trace_cap=1)
    dt = time.perf_counter() - t0
    return dict(jobs=jobs, searches_per_s=jobs / dt, instances_per_s=jobs / dt / len(off))


def kernel_split(sizes):
    """Runs the GPU part under rocprofv3 (kernel trace + stats, nothing else) and sums kernel time by phase."""
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    out = tempfile.mkdtemp(prefix="bench_labels_")
    cmd = [exe, "--kernel-trace", "--stats", "-d", out, "-o", "labels", "--output-format", "csv", "--",
           sys.executable, os.path.abspath(__file__), "--sizes", ",".join(map(str, sizes)), "--gpu_only", "--repeat", "1"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=1200)
    files = glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True)
    if p.returncode != 0 or not files:
        return dict(error=f"rocprofv3 exit {p.returncode}", tail=(p.stderr or p.stdout)[-500:])
    phases = dict(expansion=0.0, search=0.0, labelling=0.0, other=0.0)
    kernels = {}
    with open(files[0]) as f:
        for row in csv.DictReader(f):
            name, ns = row["Name"], float(row["TotalDurationNs"])
            kernels[name[:80]] = ns * 1e-9
            if "label_expand" in name or "tour_cost" in name:
                phases["expansion"] += ns * 1e-9
            elif "label_" in name:
                phases["labelling"] += ns * 1e-9
            elif "gls" in name or "symmetry" in name or "neighbor_lists" in name:
                phases["search"] += ns * 1e-9
            else:
                phases["other"] += ns * 1e-9
    total = sum(phases.values())
    shutil.rmtree(out, ignore_errors=True)
    return dict(seconds=phases, share={k: v / total for k, v in phases.items()} if total > 0 else {},
                note="kernel time of the whole GPU part (all sizes, base searches included in 'search')")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="20,50,100")
    ap.add_argument("--repeat", type=int, default=2)
    ap.add_argument("--rocprof", action="store_true")
    ap.add_argument("--gpu_only", action="store_true")
    args = ap.parse_args()
    sizes = [int(s) for s in args.sizes.split(",")]
    from gnngls_amd import labels
    res = dict(metric="fixed-edge searches per second (one labelling round, default budget)", label_iters=labels.LABEL_ITERS,
               perturbation_moves=labels.PERTURBATION_MOVES, gpu=gpu_rates(sizes, args.repeat))
    if not args.gpu_only:
        res["cpu_oracle_one_core"] = {n: cpu_rate(n) for n in sizes}
    if args.rocprof:
        res["kernel_split"] = kernel_split(sizes)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
