"""Regenerates tests/golden/train_plan_grid.npz: what one training step (forward in training mode + backward) launched and computed on
an MI355X, over the smallest shapes at which each of its launch decisions can flip, at the commit named in the file (`commit`) --
before those decisions moved into csrc/model_plan.cpp (train_plan).

    python tests/golden/make_train_plan_fixture.py [--commit HASH] [--out FILE]

One fresh child process (train_plan_child.py) per setting of SETTINGS, one after the other, each under a time limit of its own; the
first non-zero exit ends the recording.
  points                          (n, n_heads, n_layers, in_dim, B) of every grid point, the order of the arrays below
  recorded[setting, point]        whether the setting runs the point (the forced head split: 8 heads only)
  spans[setting, point, kind]     profile spans per kind of KINDS after one forward + backward
  digests[setting, point, what]   SHA-256 of the bytes of y_out, bn_batch_stats [n_layers][4][128] and the whole gradient image
  kept, kept_y<k>, kept_stats<k>  indices into `points` whose y_out and bn_batch_stats are stored whole, [setting, ...] each (default
  kept_grads, kept_grads<k>       setting only), and those whose gradient image is
Parameters: numpy.random.default_rng(seed) normals times 0.05 over the whole packed image; features uniform in [0, 1); dy standard
normals.  The child asserts that every output is finite and that a second pass over the grid repeats every span and digest (the
step has no atomics)."""
import itertools
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
GOLDEN = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(GOLDEN, "train_plan_grid.npz")
CHILD = os.path.join(GOLDEN, "train_plan_child.py")

SMALL_N = [3, 4, 17, 18, 65, 66]                      # full cross product: the 16- and 64-source tile edges
# B = 1, one layer, in_dim 1: the K1 head split (116 | 117), backward tiles 9 -> 13 (145 | 146) and 13 -> 16 (209 | 210), the limit
# (257: M = 32,896 rows, beyond the 256 chunks of gemm_tn_chunks)
LARGE_N = [116, 117, 145, 146, 209, 210, 257]
HEADS = [1, 2, 4, 8, 16]
LAYERS = [0, 1, 2]
IN_DIMS = [1, 2]
BATCHES = [1, 2]
EXTRA = [(257, 8, 1, 1, 2)]                            # M = 65,792 rows: beyond the 512 blocks of colsum_blocks
# (name, environment, head counts it runs at)
SETTINGS = [("default", {}, HEADS), ("gat_heads_4", {"GNNGLS_GAT_HEADS": "4"}, [8])]
SWITCH_VARS = ("GNNGLS_FFN_FP32", "GNNGLS_GAT_RANK1", "GNNGLS_GAT_HEADS")
KINDS = ["embed", "gemm_fc", "gat_rows", "decision", "ffn_fused", "train_colsum", "train_elementwise", "train_gemm_bwd", "train_gemm_tn",
         "train_gat_bwd"]
KIND_INDEX = [1, 2, 3, 7, 12, 13, 14, 15, 16, 17]     # GNNGLS_PROF_* of KINDS
N_PROF_KINDS = 20
WHAT = ["y_out", "bn_batch_stats", "grads"]
KEPT = [(3, 8, 1, 1, 1), (4, 16, 2, 2, 2), (17, 1, 1, 1, 2), (18, 4, 2, 2, 1), (18, 2, 1, 1, 1), (65, 8, 2, 1, 1), (66, 16, 1, 2, 1)]
KEPT_GRADS = [(3, 8, 1, 1, 1), (18, 16, 0, 2, 2), (66, 4, 0, 1, 1)]     # (a layer's gradients are 0.6 MB)
CHILD_TIMEOUT_S = 300
BN_EPS = 1e-5


def pairs(n):
    return n * (n - 1) // 2


def grid_points():
    """Every grid point as (n, n_heads, n_layers, in_dim, B)."""
    pts = list(itertools.product(SMALL_N, HEADS, LAYERS, IN_DIMS, BATCHES))
    pts += list(itertools.product(LARGE_N, HEADS, [1], [1], [1]))
    return pts + EXTRA


def run_children(outdir, python=sys.executable):
    """The children, one after the other, each a fresh process under its own time limit; stops at the first that exits non-zero
    (nothing is started after it, nothing is retried).  -> (name of the child that failed or None, its output, [child result files])"""
    files = []
    for name, switches, _ in SETTINGS:
        env = {k: v for k, v in os.environ.items() if k not in SWITCH_VARS}
        env.update(switches)
        path = os.path.join(outdir, f"train_plan_{name}.npz")
        out = subprocess.run(["timeout", "-k", "10", str(CHILD_TIMEOUT_S), python, CHILD, name, path], env=env, cwd=ROOT,
                             stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if out.returncode != 0:
            return name, f"exit {out.returncode}\n{out.stdout[-4000:]}", files
        files.append(path)
    return None, "", files


def load_device(files):
    """The children's result files -> the fixture's arrays."""
    pts = grid_points()
    recorded = np.zeros((len(SETTINGS), len(pts)), np.uint8)
    spans = np.zeros((len(SETTINGS), len(pts), len(KINDS)), np.int16)
    digests = np.zeros((len(SETTINGS), len(pts), len(WHAT), 32), np.uint8)
    out = {}
    for s, path in enumerate(files):
        with np.load(path) as z:
            idx = z["index"]
            assert idx.tolist() == [i for i, p in enumerate(pts) if p[1] in SETTINGS[s][2]]
            recorded[s, idx], spans[s, idx], digests[s, idx] = 1, z["spans"], z["digests"]
            if s == 0:
                for k in range(len(KEPT)):
                    out[f"kept_y{k}"], out[f"kept_stats{k}"] = z[f"y{k}"], z[f"stats{k}"]
                for k in range(len(KEPT_GRADS)):
                    out[f"kept_grads{k}"] = z[f"grads{k}"]
    out.update({"points": np.asarray(pts, np.int16), "settings": np.asarray([name for name, _, _ in SETTINGS]), "recorded": recorded,
                "spans": spans, "digests": digests, "kept": np.asarray([pts.index(p) for p in KEPT], np.int32),
                "kept_grads": np.asarray([pts.index(p) for p in KEPT_GRADS], np.int32)})
    return out


DEVICE_KEYS = (["points", "settings", "recorded", "spans", "digests", "kept", "kept_grads"] + [f"kept_y{k}" for k in range(len(KEPT))] +
               [f"kept_stats{k}" for k in range(len(KEPT))] + [f"kept_grads{k}" for k in range(len(KEPT_GRADS))])


def main():
    import argparse
    import tempfile
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", help="the commit the library was built from (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=FIXTURE)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("the training step's fixture is recorded on a GPU")
    with tempfile.TemporaryDirectory() as tmp:
        failed, output, files = run_children(tmp)
        if failed:
            sys.exit(f"child {failed} failed: {output}")
        arrays = load_device(files)
    commit = args.commit or subprocess.check_output(["git", "rev-parse", "HEAD"], cwd=ROOT).decode().strip()
    np.savez_compressed(args.out, commit=np.asarray(commit), **arrays)
    print(os.path.basename(args.out), os.path.getsize(args.out), "bytes,", commit)


if __name__ == "__main__":
    main()
