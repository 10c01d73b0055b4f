#!/usr/bin/env python
"""Randomised parity campaign of the training step: random instance sizes, batch sizes and data seeds; every gradient
tensor of the HIP path and of the fp32 CPU oracle against the fp64 oracle.  Prints, per case, the relative L2 error of the
whole gradient and the worst per-tensor relative L2 / max errors of both, and checks the same bounds as
tests/test_train_gpu.py.

    python scripts/train_parity_campaign.py [--cases 20] [--seed 1] [--max_n 40] [--n_heads 8]

--n_heads H (1, 2, 4 or 16): the model of H heads x 128/H features and H layers (tests/test_heads_gpu.py::make_models).
"""
import argparse
import copy
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_train_gpu as T  # noqa: E402
import test_heads_gpu as TH  # noqa: E402
from oracle import model_oracle as mo  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=20)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--max_n", type=int, default=40)
    ap.add_argument("--n_heads", type=int, default=8)
    args = ap.parse_args()
    rng = np.random.default_rng(args.seed)
    t0, failed, stats = time.time(), 0, []
    for _ in range(args.cases):
        n, B = int(rng.integers(3, args.max_n + 1)), int(rng.integers(1, 5))
        if args.n_heads == 8:
            model, oracle = T.make_models(4321, 77)
        else:
            model, oracle, _ = TH.make_models(args.n_heads, seed=4321, sd_seed=77)
        oracle64 = copy.deepcopy(oracle).double()
        N = n * (n - 1) // 2
        drng = np.random.default_rng(int(rng.integers(1 << 30)))
        x = torch.from_numpy(drng.random((B * N, 1)).astype(np.float32))
        t = torch.from_numpy(drng.random((B * N, 1)).astype(np.float32))
        G = mo.batch_line_graphs(n, B)
        _, _, g32, _ = mo.train_step_reference(oracle, G, x, t)
        _, _, g64, _ = mo.train_step_reference(oracle64, G, x.double(), t.double())
        _, _, gh, _ = T.hip_step(model, n, B, x, t)
        m = T.gradient_error_metrics(gh, g32, g64)
        ok = T.gradient_errors_acceptable(m)
        failed += not ok
        stats.append((m["global_l2_hip"], m["global_l2_32"], m["worst_max_hip"], m["worst_max_32"]))
        print(f"n={n:3d} B={B} {'ok  ' if ok else 'FAIL'} global L2 hip {m['global_l2_hip']:.1e} fp32 {m['global_l2_32']:.1e} | "
              f"worst tensor L2 hip {m['worst_l2_hip']:.1e} fp32 {m['worst_l2_32']:.1e} | worst max-rel hip {m['worst_max_hip']:.1e} "
              f"fp32 {m['worst_max_32']:.1e} | median max-rel hip {m['median_max_hip']:.1e} fp32 {m['median_max_32']:.1e}")
    a = np.array(stats)
    med, p90 = np.median(a, axis=0), np.quantile(a, 0.9, axis=0)
    print(f"n_heads={args.n_heads}: {args.cases} random (n, batch) training steps, {time.time() - t0:.0f} s; whole-gradient relative L2 error: median hip "
          f"{med[0]:.1e} / fp32 oracle {med[1]:.1e}, 90th percentile hip {p90[0]:.1e} / fp32 oracle {p90[1]:.1e}; worst entry error "
          f"(of max|g|): median hip {med[2]:.1e} / fp32 oracle {med[3]:.1e}; {failed} cases outside the per-case bounds "
          "(a kink flip on one side only)")
    # the claim is distributional: the HIP gradients are as close to the exact ones as an fp32 evaluation of the reference graph
    sys.exit(0 if med[0] <= 1.5 * med[1] and p90[0] <= 2 * p90[1] else 1)


if __name__ == "__main__":
    main()
