"""The training step's plan and workspace layout (csrc/model_plan.cpp: train_plan, train_layout) alone -- plain C++, compiled here with
the host compiler under AddressSanitizer + UndefinedBehaviorSanitizer into tests/train_plan_sweep.cpp, a process of its own -- against
what the C ABI answered before the plan existed (tests/golden/forward_plan_grid.npz: `tw_bytes_heads` over the size axes, and the
return code of every refused training call):

* over the size axes the layout's end + 256 and the size query equal the recorded bytes, and the plan's status follows the documented
  order of refusals (head count, bad argument, n beyond 257, workspace too small);
* every recorded refusal of a training call gets the recorded code from the plan (a NULL `dy` / `bn_batch_stats` is refused behind it);
* wherever a layout exists the sweep itself checks it: regions ascending, 256-byte aligned, without overlap or gap, PMS / ATT / DLR
  twice as wide at 16 heads, TNP sized by gemm_tn_chunks(M), and every accepted plan against the policy's rules.
tests/golden/train_plan_grid.npz (what the step launched and computed on an MI355X before the plan) covers the grid it names."""
import itertools
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import make_forward_plan_fixture as mk  # noqa: E402
import make_train_plan_fixture as mt  # noqa: E402

OK, TRAIN_WORKSPACE_SMALL = 0, 4


@pytest.fixture(scope="module")
def golden():
    with np.load(mk.FIXTURE) as z:
        return {k: z[k] for k in ("size_n", "size_B", "size_heads", "size_layers", "tw_bytes_heads", "ref_call", "ref_rc")}


def documented_status(B, n, layers, H, in_dim=1):
    if H not in (1, 2, 4, 8, 16):
        return mk.ERR_UNSUPPORTED
    if B < 1 or n < 3 or in_dim < 1 or layers < 0:
        return mk.ERR_ARG
    return mk.ERR_UNSUPPORTED if n > 257 else OK


def test_plan_unit_alone_under_asan_ubsan(golden, tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++")
    assert cxx, "no host C++ compiler"
    exe, grid = str(tmp_path / "train_plan_sweep"), str(tmp_path / "grid.txt")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "train_plan_sweep.cpp"),
                           os.path.join(ROOT, "gnngls_amd", "csrc", "model_plan.cpp"), "-o", exe])
    axes = list(itertools.product(golden["size_B"].tolist(), golden["size_n"].tolist(), golden["size_layers"].tolist(),
                                  golden["size_heads"].tolist()))
    accepted = [a for a in axes if documented_status(*a) == OK]
    calls = [(desc, a) for desc, entry, a in mk.refused_calls() if entry.startswith("train_")]
    assert [d for d, _ in calls] == [d for d in golden["ref_call"].tolist() if ": train_" in d] and calls and accepted
    # n B in_dim n_layers n_heads pointers_given workspace_mode gat_heads
    lines = [(n, B, 1, layers, H, 1, 0, 0) for B, n, layers, H in axes]
    lines += [(n, B, 1, layers, H, 1, mode, 0) for B, n, layers, H in accepted for mode in (1, 2)]
    lines += [(n, B, 1, layers, 8, 1, 0, forced) for B, n, layers, H in accepted if H == 8 for forced in (4, 8)]
    lines += [(a["n"], a["B"], a["in_dim"], a["layers"], a["H"], int(a["null"] in (None, "extra")), {"full": 0, "short": 1, "zero": 2}[a["ws"]], 0)
              for _, a in calls]
    with open(grid, "w") as f:
        f.write("".join(" ".join(map(str, line)) + "\n" for line in lines))
    out = subprocess.run([exe, grid], capture_output=True, timeout=600)
    assert out.returncode == 0 and not out.stderr, out.stderr.decode()[-3000:]
    rec = np.frombuffer(out.stdout, dtype=np.int64).reshape(len(lines), 4)
    # the size axes: the recorded bytes from the size query and from the layout, the documented status
    want = golden["tw_bytes_heads"].reshape(-1)
    assert want.size == len(axes) and (want > 0).any() and (want == 0).any()
    for col, name in ((0, "train_workspace_bytes"), (1, "train_layout().end + 256")):
        bad = np.argwhere(rec[:len(axes), col] != want).reshape(-1)
        assert bad.size == 0, f"{name}: {len(bad)} points differ, first (B, n, layers, heads) = {axes[int(bad[0])]}: {rec[int(bad[0]), col]} != {want[int(bad[0])]}"
    for i, a in enumerate(axes):
        assert rec[i, 2] == documented_status(*a), f"(B, n, layers, heads) = {a}: status {rec[i, 2]}"
    k = len(axes)
    short = rec[k:k + 2 * len(accepted)]
    assert (short[:, 2] == mk.ERR_ARG).all() and (short[:, 3] == TRAIN_WORKSPACE_SMALL).all()
    k += 2 * len(accepted)
    forced = rec[k:len(lines) - len(calls)]
    assert len(forced) and (forced[:, 2] == OK).all()
    # the recorded refusals
    codes = dict(zip(golden["ref_call"].tolist(), golden["ref_rc"].tolist()))
    for (desc, a), r in zip(calls, rec[len(lines) - len(calls):]):
        if a["null"] == "extra":        # dy / bn_batch_stats: refused by the entry point behind an accepted plan
            assert r[2] == OK and codes[desc] == mk.ERR_ARG, desc
        else:
            assert r[2] == codes[desc] != OK, f"{desc}: status {r[2]} != {codes[desc]}"


def test_device_fixture_covers_the_grid_it_names():
    with np.load(mt.FIXTURE) as z:
        g = {k: z[k] for k in z.files}
    assert sorted(g) == sorted(["commit"] + mt.DEVICE_KEYS) and len(str(g["commit"])) == 40
    pts = mt.grid_points()
    assert g["points"].tolist() == [list(p) for p in pts] and g["settings"].tolist() == [name for name, _, _ in mt.SETTINGS]
    have = {tuple(p) for p in pts}
    for H in mt.HEADS:            # (n, n_heads, n_layers, in_dim, B): the edges of every launch decision, at every head count
        assert {(n, H, 1, 1, 1) for n in (116, 117, 145, 146, 209, 210, 257)} <= have
        assert {(n, H, layers, d, B) for n in (3, 4, 17, 18, 65, 66) for layers in (0, 1, 2) for d in (1, 2) for B in (1, 2)} <= have
    assert (257, 8, 1, 1, 2) in have
    spans = g["spans"]
    assert spans.shape == (len(mt.SETTINGS), len(pts), len(mt.KINDS)) and g["digests"].shape == (len(mt.SETTINGS), len(pts), len(mt.WHAT), 32)
    recorded = g["recorded"].astype(bool)      # [setting, point]: the forced-split setting runs at 8 heads only
    for s, (_, _, heads) in enumerate(mt.SETTINGS):
        assert recorded[s].tolist() == [p[1] in heads for p in pts]
    layers = np.asarray([p[2] for p in pts])
    gat_fwd, gat_bwd = spans[0, :, mt.KINDS.index("gat_rows")], spans[0, :, mt.KINDS.index("train_gat_bwd")]
    assert (gat_fwd == layers).all() and (gat_bwd == layers).all()
    whole = [g[k] for k in mt.DEVICE_KEYS if k.startswith("kept_") and k != "kept_grads"]
    assert len(whole) == 2 * len(mt.KEPT) + len(mt.KEPT_GRADS) and all(a.size and np.isfinite(a).all() for a in whole)
