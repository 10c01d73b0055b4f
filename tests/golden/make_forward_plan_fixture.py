"""Regenerates tests/golden/forward_plan_grid.npz: what the regret model's forward did, over the smallest shapes at which each of
its launch decisions can flip, at the commit named in the file (`commit`) -- before those decisions moved into csrc/model_plan.cpp.

    python tests/golden/make_forward_plan_fixture.py [--commit HASH] [--out FILE]

Host part (no GPU needed; a refused call reads none of its pointers):
  pf_*, pb_*, fw_*, tw_*        gnngls_model_packed_floats, gnngls_regret_prepared_bytes, gnngls_regret_forward_workspace_bytes[_heads],
                                gnngls_regret_train_workspace_bytes[_heads] over the axes stored beside them
  ref_call, ref_rc, ref_text    every refused forward / prepare / training call of refused_calls(): its description, return code and
                                gnngls_last_error() text
Device part (an MI355X; kept from the existing file where there is no GPU): one fresh child process (forward_plan_child.py) per switch
setting of SETTINGS, one after the other, each under a time limit of its own; the first non-zero exit ends the recording.
  points                        (n, n_heads, n_layers, in_dim, form, bmode) of every accepted point, the order of the arrays below
  spans[setting, point, kind]   profile spans per kind of KINDS after one forward
  digest_index[setting, point]  row of `digests` holding the SHA-256 of y_out's bytes
  kept, kept_y<k>               indices into `points` whose y_out is stored whole, [setting, B * N] each
Weights: numpy.random.default_rng(seed) normals times 0.05 over the whole packed image; features uniform in [0, 1).  The child asserts
that every y_out is finite and that a second pass over the grid repeats every digest (the forward has no atomics)."""
import ctypes
import itertools
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
GOLDEN = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(GOLDEN, "forward_plan_grid.npz")
CHILD = os.path.join(GOLDEN, "forward_plan_child.py")

# ---- the grid ---------------------------------------------------------------------------------------------------------------
SMALL_N = [3, 4, 17, 18, 65, 66]                                     # full cross product
LARGE_N = [116, 117, 129, 130, 193, 194, 255, 256, 257, 258]          # B = 1, one layer
HEADS = [1, 2, 4, 8, 16]
LAYERS = [0, 1, 3]
IN_DIMS = [1, 2, 32, 33]
LARGE_IN_DIMS = [1, 2]
FORM_ONE_CALL, FORM_PREPARED, FORM_PREPARED_NULL = 0, 1, 2
FORMS = [FORM_ONE_CALL, FORM_PREPARED, FORM_PREPARED_NULL]
# bmode 0: B = 1, the full workspace; 1: B = 3 in workspace_bytes(2, n) (chunks of 2 + 1); 2: B = 3, the workspace pointer 4 bytes
# behind a 256-byte boundary (the alignment slack)
BMODES = [0, 1, 2]
SETTINGS = [("default", {}), ("ffn_fp32", {"GNNGLS_FFN_FP32": "1"}), ("rank1_0", {"GNNGLS_GAT_RANK1": "0"}),
            ("rank1_2", {"GNNGLS_GAT_RANK1": "2"})]
SWITCH_VARS = ("GNNGLS_FFN_FP32", "GNNGLS_GAT_RANK1", "GNNGLS_GAT_HEADS")
KINDS = ["embed", "gemm_fc", "gat_rows", "gat_rows_rank1", "ffn_fused", "decision"]
KIND_INDEX = [1, 2, 3, 4, 12, 7]                                      # GNNGLS_PROF_* of KINDS
N_PROF_KINDS = 20
KEPT = [(3, 8, 1, 1, 1, 0), (4, 16, 3, 2, 0, 1), (17, 8, 3, 1, 1, 1), (17, 4, 1, 32, 1, 2), (18, 8, 0, 1, 1, 0), (18, 1, 3, 33, 2, 1),
        (18, 16, 1, 1, 1, 2), (18, 2, 3, 2, 0, 0), (65, 8, 1, 1, 1, 0), (66, 8, 3, 2, 1, 0)]
CHILD_TIMEOUT_S = 240
ERR_ARG, ERR_UNSUPPORTED = -1, -3

# host-only axes
SIZE_N = [2] + SMALL_N + LARGE_N + [423, 424, 65535, 65536]
SIZE_B = [0, 1, 2, 3]
SIZE_HEADS = [1, 2, 3, 4, 8, 16, 32]
SIZE_LAYERS = [-1, 0, 1, 3]
SIZE_IN_DIMS = [-1, 0, 1, 2, 32, 33]


def pairs(n):
    return n * (n - 1) // 2


def batch_of(bmode):
    return 1 if bmode == 0 else 3


def grid_points():
    """Every grid point as (n, n_heads, n_layers, in_dim, form, bmode)."""
    pts = list(itertools.product(SMALL_N, HEADS, LAYERS, IN_DIMS, FORMS, BMODES))
    pts += list(itertools.product(LARGE_N, HEADS, [1], LARGE_IN_DIMS, FORMS, [0]))
    return pts


def accepted(p):
    """The documented limits: 8 heads reach n = 423, the other head counts n = 257."""
    n, H = p[0], p[1]
    return 3 <= n <= (423 if H == 8 else 257)


def accepted_points():
    return [p for p in grid_points() if accepted(p)]


# ---- host part --------------------------------------------------------------------------------------------------------------
def record_sizes(L):
    out = {"size_n": np.asarray(SIZE_N, np.int32), "size_B": np.asarray(SIZE_B, np.int8), "size_heads": np.asarray(SIZE_HEADS, np.int8),
           "size_layers": np.asarray(SIZE_LAYERS, np.int8), "size_in_dims": np.asarray(SIZE_IN_DIMS, np.int8)}
    out["pf_floats"] = np.asarray([[L.gnngls_model_packed_floats(d, l) for l in SIZE_LAYERS] for d in SIZE_IN_DIMS], np.int64)
    out["pb_bytes"] = np.asarray([L.gnngls_regret_prepared_bytes(l) for l in SIZE_LAYERS], np.int64)
    out["fw_bytes"] = np.asarray([[L.gnngls_regret_forward_workspace_bytes(b, n) for n in SIZE_N] for b in SIZE_B], np.int64)
    out["fw_bytes_heads"] = np.asarray([[[L.gnngls_regret_forward_workspace_bytes_heads(b, n, h) for h in SIZE_HEADS] for n in SIZE_N]
                                        for b in SIZE_B], np.int64)
    out["tw_bytes"] = np.asarray([[[L.gnngls_regret_train_workspace_bytes(b, n, l) for l in SIZE_LAYERS] for n in SIZE_N]
                                  for b in SIZE_B], np.int64)
    out["tw_bytes_heads"] = np.asarray([[[[L.gnngls_regret_train_workspace_bytes_heads(b, n, l, h) for h in SIZE_HEADS]
                                          for l in SIZE_LAYERS] for n in SIZE_N] for b in SIZE_B], np.int64)
    return out


def forward_desc(tag, n, H, layers, in_dim, form, B=1, ws="full", pb="full", plain=False, null=None):
    return f"{tag}: forward n={n} H={H} L={layers} d={in_dim} form={form} B={B} ws={ws} pb={pb} plain={int(plain)} null={null}"


def grid_refusal_desc(p):
    """The description under which the refusal of a grid point that is not accepted() is recorded."""
    return forward_desc("grid", p[0], p[1], p[2], p[3], p[4], B=batch_of(p[5]))


def refused_calls():
    """-> [(description, entry, kwargs)]: calls the host refuses before any device work.  The one-call forward is only listed where it
    makes no scratch image first (n_layers == 0, bad arguments, a head count other than 8 beyond its n)."""
    calls = []

    def fwd(tag, n, H, layers, in_dim, form, B=1, ws="full", pb="full", plain=False, null=None):
        calls.append((forward_desc(tag, n, H, layers, in_dim, form, B, ws, pb, plain, null),
                      "forward", dict(n=n, H=H, layers=layers, in_dim=in_dim, form=form, B=B, ws=ws, pb=pb, plain=plain, null=null)))

    for p in grid_points():
        if not accepted(p):
            fwd("grid", p[0], p[1], p[2], p[3], p[4], B=batch_of(p[5]))

    def train(tag, which, n, H, layers, in_dim, B=1, ws="full", plain=False, null=None):
        calls.append((f"{tag}: train_{which} n={n} H={H} L={layers} d={in_dim} B={B} ws={ws} plain={int(plain)} null={null}",
                      "train_" + which, dict(n=n, H=H, layers=layers, in_dim=in_dim, B=B, ws=ws, plain=plain, null=null)))

    for form in FORMS:
        for plain in (False, True):
            fwd("n below 3", 2, 8, 1 if form else 0, 1, form, plain=plain)
            fwd("K1 limit", 424, 8, 1 if form else 0, 1, form, plain=plain)
            fwd("in_dim 0", 10, 8, 1, 0, form, plain=plain)
            fwd("negative layers", 10, 8, -1, 1, form, plain=plain)
            fwd("negative batch", 10, 8, 1, 1, form, B=-1, plain=plain)
            for null in ("feat", "weights", "y_out", "workspace"):
                fwd("null pointer", 10, 8, 1, 1, form, plain=plain, null=null)
        for H in (1, 2, 4, 16):
            for layers in LAYERS:
                fwd("K1h limit", 258, H, layers, 1, form)
            fwd("n below 3", 2, H, 1 if form else 0, 1, form)
            fwd("in_dim 0", 10, H, 1, 0, form)
        for H in (0, 3, 32):
            fwd("head count", 10, H, 1, 1, form)
            fwd("head count beyond n", 300, H, 1, 1, form)
    for n, H in itertools.product([3, 18, 66, 423], HEADS):
        if not accepted((n, H)):
            continue
        for form, layers in [(FORM_ONE_CALL, 0), (FORM_PREPARED, 0), (FORM_PREPARED, 3), (FORM_PREPARED_NULL, 1)]:
            for ws in ("short", "short_slack", "zero"):
                fwd("workspace", n, H, layers, 1, form, B=3, ws=ws, plain=H == 8)
    for layers, H in itertools.product([0, 1, 3], [4, 8]):
        fwd("prepared image", 18, H, layers, 2, FORM_PREPARED, pb="short", plain=H == 8)
        fwd("prepared image", 18, H, layers, 2, FORM_PREPARED, pb="zero")
    fwd("image before workspace", 18, 8, 1, 2, FORM_PREPARED, ws="short", pb="short")
    fwd("n before image", 424, 8, 1, 2, FORM_PREPARED, pb="short")
    for which in ("forward", "backward"):
        for plain in (False, True):
            train("n below 3", which, 2, 8, 1, 1, plain=plain)
            train("in_dim 0", which, 10, 8, 1, 0, plain=plain)
            train("empty batch", which, 10, 8, 1, 1, B=0, plain=plain)
            train("backward limit", which, 258, 8, 1, 1, plain=plain)
            train("workspace", which, 18, 8, 3, 1, B=2, ws="short", plain=plain)
            for null in ("feat", "params", "io", "workspace", "extra"):
                train("null pointer", which, 10, 8, 1, 1, plain=plain, null=null)
        for H in (1, 2, 4, 16):
            train("backward limit", which, 258, H, 1, 1)
            train("workspace", which, 18, H, 3, 1, B=2, ws="short")
            train("workspace", which, 257, H, 0, 1, ws="zero")
        for H in (0, 3, 32):
            train("head count", which, 10, H, 1, 1)
    for in_dim, layers, pb in [(0, 1, "full"), (1, -1, "full"), (1, 0, "short"), (2, 3, "short"), (33, 1, "zero")]:
        for H in (None, 4, 3):
            calls.append((f"prepare d={in_dim} L={layers} pb={pb} H={H}", "prepare", dict(in_dim=in_dim, layers=layers, pb=pb, H=H)))
    return calls


def record_refusals(L):
    """Makes every call of refused_calls() with dummy pointers into a small host buffer -> (descriptions, codes, texts)."""
    buf = (ctypes.c_ubyte * 1024)()
    aligned = (ctypes.addressof(buf) + 255) & ~255
    dummy = ctypes.c_void_p(aligned + 512)
    descs, codes, texts = [], [], []
    for desc, entry, a in refused_calls():
        if entry == "prepare":
            need = L.gnngls_regret_prepared_bytes(a["layers"])
            pb = {"full": need, "short": need - 1, "zero": 0}[a["pb"]]
            if a["H"] is None:
                rc = L.gnngls_regret_prepare(dummy, a["in_dim"], a["layers"], dummy, pb, None)
            else:
                rc = L.gnngls_regret_prepare_heads(dummy, a["in_dim"], a["layers"], a["H"], dummy, pb, None)
        elif entry == "forward":
            n, H, B = a["n"], a["H"], a["B"]
            one = L.gnngls_regret_forward_workspace_bytes_heads(1, n, H) - 256          # N * bytes per node (0: not a size)
            ws_ptr, ws = aligned, max(B, 1) * one + 256
            if a["ws"] == "short":
                ws = one - 1
            elif a["ws"] == "short_slack":                                                # 252 bytes go to the alignment
                ws_ptr, ws = aligned + 4, one + 251
            elif a["ws"] == "zero":
                ws = 0
            need = L.gnngls_regret_prepared_bytes(a["layers"])
            pb = {"full": need, "short": need - 1, "zero": 0}[a["pb"]]
            p = {k: dummy for k in ("feat", "weights", "y_out")}
            p["workspace"] = ctypes.c_void_p(ws_ptr)
            if a["null"]:
                p[a["null"]] = None
            image = dummy if a["form"] == FORM_PREPARED else None
            tail = (p["y_out"], p["workspace"], ws, None)
            if a["form"] == FORM_ONE_CALL:
                if a["plain"]:
                    rc = L.gnngls_regret_forward(p["feat"], p["weights"], B, n, a["in_dim"], a["layers"], *tail)
                else:
                    rc = L.gnngls_regret_forward_heads(p["feat"], p["weights"], B, n, a["in_dim"], a["layers"], H, *tail)
            elif a["plain"]:
                rc = L.gnngls_regret_forward_prepared(p["feat"], p["weights"], image, pb, B, n, a["in_dim"], a["layers"], *tail)
            else:
                rc = L.gnngls_regret_forward_prepared_heads(p["feat"], p["weights"], image, pb, B, n, a["in_dim"], a["layers"], H, *tail)
        else:
            n, H, B, layers = a["n"], a["H"], a["B"], a["layers"]
            need = L.gnngls_regret_train_workspace_bytes_heads(B, n, layers, H)
            ws = {"full": need, "short": need - 1, "zero": 0}[a["ws"]]
            p = {k: dummy for k in ("feat", "params", "io", "workspace", "extra")}
            if a["null"]:
                p[a["null"]] = None
            if entry == "train_forward":        # io = y_out, extra = bn_batch_stats
                args = (p["feat"], p["params"], B, n, a["in_dim"], layers) + (() if a["plain"] else (H,)) + (
                    1e-5, p["io"], p["extra"], p["workspace"], ws, None)
                rc = (L.gnngls_regret_train_forward if a["plain"] else L.gnngls_regret_train_forward_heads)(*args)
            else:                               # io = grads, extra = dy
                args = (p["feat"], p["params"], p["extra"], B, n, a["in_dim"], layers) + (() if a["plain"] else (H,)) + (
                    p["io"], p["workspace"], ws, None)
                rc = (L.gnngls_regret_train_backward if a["plain"] else L.gnngls_regret_train_backward_heads)(*args)
        assert rc in (ERR_ARG, ERR_UNSUPPORTED), f"{desc}: not refused by the host (rc {rc})"
        descs.append(desc)
        codes.append(rc)
        texts.append(L.gnngls_last_error().decode())
    return descs, codes, texts


def record_host(L):
    out = record_sizes(L)
    descs, codes, texts = record_refusals(L)
    out["ref_call"], out["ref_rc"], out["ref_text"] = np.asarray(descs), np.asarray(codes, np.int8), np.asarray(texts)
    return out


# ---- device part ------------------------------------------------------------------------------------------------------------
def run_children(outdir, python=sys.executable):
    """The four children, one after the other, each a fresh process under its own time limit; stops at the first that exits non-zero
    (nothing is started after it, nothing is retried).  -> (name of the child that failed or None, its output, [child result files])"""
    files = []
    for name, switches in SETTINGS:
        env = {k: v for k, v in os.environ.items() if k not in SWITCH_VARS}
        env.update(switches)
        path = os.path.join(outdir, f"forward_plan_{name}.npz")
        out = subprocess.run(["timeout", "-k", "10", str(CHILD_TIMEOUT_S), python, CHILD, path], env=env, cwd=ROOT,
                             stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if out.returncode != 0:
            return name, f"exit {out.returncode}\n{out.stdout[-4000:]}", files
        files.append(path)
    return None, "", files


def load_device(files):
    """The children's result files -> the device part of the fixture."""
    pts = accepted_points()
    spans, digests, kept_y = [], [], []
    for path in files:
        with np.load(path) as z:
            assert z["points"].tolist() == [list(p) for p in pts]
            spans.append(z["spans"])
            digests.append(z["digests"])
            kept_y.append([z[f"y{k}"] for k in range(len(KEPT))])
    digests = np.stack(digests)                                          # [setting, point, 32]
    table, index = np.unique(digests.reshape(-1, 32), axis=0, return_inverse=True)
    out = {"points": np.asarray(pts, np.int16), "settings": np.asarray([name for name, _ in SETTINGS]),
           "spans": np.stack(spans).astype(np.int8), "digests": table, "digest_index": index.reshape(digests.shape[:2]).astype(np.int32),
           "kept": np.asarray([pts.index(p) for p in KEPT], np.int32)}
    for k in range(len(KEPT)):
        out[f"kept_y{k}"] = np.stack([ys[k] for ys in kept_y])
    return out


DEVICE_KEYS = ["points", "settings", "spans", "digests", "digest_index", "kept"] + [f"kept_y{k}" for k in range(len(KEPT))]


def main():
    import argparse
    import tempfile
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", help="the commit the library was built from (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=FIXTURE)
    args = ap.parse_args()
    import torch
    from gnngls_amd import _lib, build
    build.build()
    arrays = record_host(_lib.load())
    if torch.cuda.is_available():
        with tempfile.TemporaryDirectory() as tmp:
            failed, output, files = run_children(tmp)
            if failed:
                sys.exit(f"child {failed} failed: {output}")
            arrays.update(load_device(files))
    else:
        with np.load(FIXTURE) as z:        # no GPU here: the device part stays as recorded
            arrays.update({k: z[k] for k in DEVICE_KEYS})
            args.commit = args.commit or str(z["commit"])
    commit = args.commit or subprocess.check_output(["git", "rev-parse", "HEAD"], cwd=ROOT).decode().strip()
    np.savez_compressed(args.out, commit=np.asarray(commit), **arrays)
    print(os.path.basename(args.out), os.path.getsize(args.out), "bytes,", commit)


if __name__ == "__main__":
    main()
