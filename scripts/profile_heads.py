#!/usr/bin/env python
"""Workload for the per-kernel measurement of the attention at every head count (run under `rocprofv3 --kernel-trace --stats`):
the inference forward of B x TSPn (synthetic checkpoint, prepared path, as the pipeline runs it) and training steps of
Bt x TSPn (forward + backward, MSE), with `--n_heads` heads of 128 / n_heads features and as many layers (models.py:59-61).

    python scripts/profile_heads.py --n_heads 4 [--n 100] [--batch 1024] [--train_batch 32] [--reps 3] [--what both]

--what fwd / train: only the forward / only the training steps (one workload per profiled process: per-launch statistics of a
kernel that both use stay apart).
"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n_heads", type=int, default=8)
    ap.add_argument("--n", type=int, default=100)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--train_batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--what", choices=("both", "fwd", "train"), default="both")
    args = ap.parse_args()
    from gnngls_amd import models as M
    from oracle import model_oracle as mo
    torch.manual_seed(0)
    H, n = args.n_heads, args.n
    sd = mo.synthetic_state_dict(mo.EdgeRegretModelOracle(1, 128, 1, 3, n_heads=H), seed=5)
    model = M.EdgePropertyPredictionModel(1, 128, 1, 3, n_heads=H)
    model.load_state_dict(sd)
    model.cuda().eval()
    N = n * (n - 1) // 2
    fwd, times = float("nan"), [float("nan")]
    if args.what != "train":
        fwd = forward(M, model, args, N)
    if args.what != "fwd":
        times = train(M, model, args, N)
    print(f"n_heads={H} layers={len(model.message_passing_layers)}: forward {args.batch} x TSP{n} {1e3 * fwd:.2f} ms (wall, incl. "
          f"launch overhead); training step {args.train_batch} x TSP{n} {1e3 * min(times):.2f} ms (wall, best of {args.reps})")


def forward(M, model, args, N):
    n = args.n
    x = torch.rand(args.batch * N, 1, device="cuda")
    with torch.no_grad():
        M.regret_forward(model, x, args.batch, n)                    # warm-up (image, workspace)
        torch.cuda.synchronize()
        t0 = time.time()
        for _ in range(args.reps):
            M.regret_forward(model, x, args.batch, n)
        torch.cuda.synchronize()
    fwd = (time.time() - t0) / args.reps
    model._workspace = None
    torch.cuda.empty_cache()
    return fwd


def train(M, model, args, N):
    n = args.n
    model.train()
    G = M.LineGraph(n, batch=args.train_batch).to("cuda")
    xt = torch.rand(args.train_batch * N, 1, device="cuda")
    target = torch.rand(args.train_batch * N, 1, device="cuda")
    crit = torch.nn.MSELoss()
    times = []
    for k in range(args.reps + 1):
        torch.cuda.synchronize()
        t0 = time.time()
        model.zero_grad()
        loss = crit(model(G, xt), target)
        loss.backward()
        torch.cuda.synchronize()
        if k:
            times.append(time.time() - t0)
    return times


if __name__ == "__main__":
    main()
