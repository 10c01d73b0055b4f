#!/usr/bin/env python
"""Measures the Held-Karp 1-tree lower bound on the device (ops.one_tree_bound; oracle/one_tree.c) on the instances bench.py searches.

    python scripts/bench_bounds.py [--out profiles/one_tree_bounds.json] [--shapes 100x1024,200x256,20x1000]

Per shape (the leading instances of block 0 of the seeded test set: same generator and seed as bench.py; ub = the best-known
lengths of bench_data/, or where a size has none the best tours of a 1 s search):

* device time of one ops.one_tree_bound call for the whole batch: HIP events on the stream, warm-up first, median of --repeats
  timed calls; the mean number of 1-trees built, the shares of the three exits, the mean bracket (best_known / bound - 1) * 100
  and the launch form (ops.one_tree_describe);
* wall time of oracle.one_tree.lower_bounds on the same instances with the same ub on --workers host cores (default 16: what
  bench.py does today after its timed region), and whether every device bound has the oracle's bits.
  THE ONE CONDITION (exit status 1 if it fails): the device batch takes less time than the oracle on those cores;
* VGPRs and scratch of every instantiation of the kernel (hipcc -Rpass-analysis=kernel-resource-usage).
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from bench import available_cores, instance_range, load_best_known  # noqa: E402
from bench_constructors import device_ms  # noqa: E402
from gnngls_amd import build as hip_build  # noqa: E402
from gnngls_amd import ops, pipeline  # noqa: E402
from oracle import one_tree  # noqa: E402


def kernel_resources():
    """{instantiation: {vgprs, scratch_bytes, occupancy}} of bounds_kernels.hip, from the compiler's resource remarks."""
    src = os.path.join(hip_build.CSRC, "bounds_kernels.hip")
    with tempfile.TemporaryDirectory() as td:
        err = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + hip_build.FLAGS +
                             ["-c", src, "-o", os.path.join(td, "x.o"), "-Rpass-analysis=kernel-resource-usage"],
                             capture_output=True, text=True, cwd=hip_build.CSRC).stderr
    rows, cur = {}, None
    for line in err.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip()
            k = re.search(r"one_tree_kernel<(\d+), (true|false)>", name)
            cur = f"{k.group(1)} node(s) per lane, {'2-4 wavefronts' if k.group(2) == 'true' else 'one wavefront'}" if k else None
            if cur:
                rows[cur] = {}
            continue
        m = re.search(r"remark:\s+(VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\d+)", line)
        if m and cur:
            rows[cur][{"VGPRs": "vgprs", "ScratchSize": "scratch_bytes", "Occupancy": "occupancy_waves_per_simd"}[m.group(1).split()[0]]] = int(m.group(2))
    return rows


def measure_shape(n, B, seed, warmup, repeats, workers, max_iters):
    D_host = instance_range(seed, n, 0, B)
    bk, bk_how = load_best_known(None, n, seed, 0, B)
    if bk is None:
        # no stored lengths at this size (bench.py compares TSP20 with the exact DP): the best tours of a 1 s search on the distances
        found = pipeline.solve_batch(torch.from_numpy(D_host).cuda(), guides=("weight",), time_limit=1.0, perturbation_moves=20)
        bk, bk_how = found.best_cost.cpu().numpy(), f"{bk_how}: best_cost of solve_batch(guides=('weight',), time_limit=1.0)"
    D, ub = torch.from_numpy(D_host).cuda(), torch.from_numpy(np.ascontiguousarray(bk, dtype=np.float64)).cuda()
    ms, raw = device_ms(lambda: ops.one_tree_bound(D, ub, max_iters=max_iters, want_pi=True), warmup, repeats)
    r = ops.one_tree_bound(D, ub, max_iters=max_iters)
    bound, kind = r.bound.cpu().numpy(), r.exit_kind.cpu().numpy()
    t0 = time.time()
    ref = one_tree.lower_bounds(D_host, bk, workers=workers, max_iters=max_iters)
    oracle_s = time.time() - t0
    return {"n": n, "instances": B, "best_known": bk_how, "max_iters": max_iters, "form": ops.one_tree_describe(n),
            "device_ms_median": ms, "device_ms_all": raw,
            "mean_iters": float(r.iters.double().mean()),
            "exit_share": {"iters": float((kind == ops.BOUND_EXIT_ITERS).mean()), "step": float((kind == ops.BOUND_EXIT_STEP).mean()),
                           "tour": float((kind == ops.BOUND_EXIT_TOUR).mean())},
            "mean_bracket_pct": float(((bk / bound - 1.0) * 100.0).mean()),
            "bound_above_best_known_instances": int((bound > bk * (1 + 1e-9)).sum()),
            "oracle_wall_s": oracle_s, "oracle_workers": workers,
            "bit_equal_to_oracle_instances": int((bound.view(np.uint64) == ref.view(np.uint64)).sum()),
            "oracle_over_device": oracle_s * 1e3 / ms, "device_faster_than_oracle": bool(ms < oracle_s * 1e3)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "one_tree_bounds.json"))
    ap.add_argument("--shapes", default="100x1024,200x256,20x1000", help="comma-separated n x instances")
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--max_iters", type=int, default=2000)
    ap.add_argument("--workers", type=int, default=0, help="host cores of the oracle (0 = min(16, the cores this process may use))")
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error("--repeats must be >= 5 (medians)")
    workers = args.workers or min(16, available_cores())
    res = {"command": f"python scripts/bench_bounds.py --shapes {args.shapes} --seed {args.seed} --warmup {args.warmup} "
                      f"--repeats {args.repeats} --max_iters {args.max_iters}", "device": torch.cuda.get_device_name(0), "seed": args.seed,
           "timing": f"HIP events on the stream, {args.warmup} warm-up calls, median of {args.repeats}; oracle: wall time of "
                     f"oracle.one_tree.lower_bounds on {workers} host processes (start-up of the pool included)",
           "kernel_resources": kernel_resources(), "shapes": []}
    for shape in args.shapes.split(","):
        n, B = (int(x) for x in shape.split("x"))
        res["shapes"].append(measure_shape(n, B, args.seed, args.warmup, args.repeats, workers, args.max_iters))
    res["condition"] = "the device batch takes less time than oracle/one_tree.c on the host cores for the same instances"
    res["condition_holds"] = all(s["device_faster_than_oracle"] for s in res["shapes"])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({"condition_holds": res["condition_holds"], "kernel_resources": res["kernel_resources"],
                      "shapes": [{k: s[k] for k in ("n", "instances", "device_ms_median", "oracle_wall_s", "oracle_over_device",
                                                    "mean_iters", "exit_share", "mean_bracket_pct", "bit_equal_to_oracle_instances")}
                                 for s in res["shapes"]]}))
    return 0 if res["condition_holds"] else 1


if __name__ == "__main__":
    sys.exit(main())
