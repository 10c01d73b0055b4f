"""The training step launches and computes what it did before its launch decisions became one function (csrc/model_plan.cpp:
train_plan): tests/golden/train_plan_grid.npz holds the profile spans per kind and the SHA-256 of y_out, bn_batch_stats and the whole
gradient image after one forward + backward at every grid point, recorded on an MI355X at the commit named in the file.  The same
child processes (tests/golden/train_plan_child.py: the default setting and the forced K1 head split, one after the other, each under
its own time limit) run here; spans and digests equal the fixture at every point -- no tolerance, the step has no atomics."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import make_train_plan_fixture as mt  # noqa: E402


@pytest.mark.gpu
def test_training_step_spans_and_outputs_as_recorded(tmp_path):
    failed, output, files = mt.run_children(str(tmp_path))      # stops at the first child that exits non-zero
    assert failed is None, f"child {failed}: {output}"
    now = mt.load_device(files)
    with np.load(mt.FIXTURE) as z:
        golden = {k: z[k] for k in mt.DEVICE_KEYS}
    pts = golden["points"].tolist()
    assert now["points"].tolist() == pts and (now["recorded"] == golden["recorded"]).all()
    assert now["kept"].tolist() == golden["kept"].tolist() and now["kept_grads"].tolist() == golden["kept_grads"].tolist()
    problems = []
    for s, (name, _, _) in enumerate(mt.SETTINGS):
        bad = np.argwhere((now["spans"][s] != golden["spans"][s]).any(axis=1)).reshape(-1)
        if bad.size:
            i = int(bad[0])
            problems.append(f"{name}: spans differ at {len(bad)} points, first {pts[i]}: {now['spans'][s, i].tolist()} != "
                            f"{golden['spans'][s, i].tolist()} ({mt.KINDS})")
        for k, what in enumerate(mt.WHAT):
            bad = np.argwhere((now["digests"][s, :, k] != golden["digests"][s, :, k]).any(axis=1)).reshape(-1)
            if bad.size:
                problems.append(f"{name}: {what} differs at {len(bad)} points, first {pts[int(bad[0])]}")
    for key in mt.DEVICE_KEYS:
        if key.startswith("kept_") and key != "kept_grads":
            a, a0 = now[key], golden[key]
            diff = np.argwhere(a.view(np.uint32) != a0.view(np.uint32)).reshape(-1)
            if diff.size:
                e = int(diff[0])
                problems.append(f"{key}: {len(diff)} of {a.size} elements differ, first [{e}] = {a[e]!r} != {a0[e]!r}")
    print("\n".join(problems))
    assert not problems, "\n".join(problems[:20])
