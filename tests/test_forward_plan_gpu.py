"""The regret forward launches and computes what it did before its launch policy became one function (csrc/model_plan.cpp):
tests/golden/forward_plan_grid.npz holds the profile spans per kind and the SHA-256 of y_out at every accepted grid point under the
four experiment-switch settings, recorded on an MI355X at the commit named in the file.  The same four child processes
(tests/golden/forward_plan_child.py, one per setting, one after the other, each under its own time limit) run here; spans and
digests equal the fixture at every point -- no tolerance, the forward has no atomics."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import make_forward_plan_fixture as mk  # noqa: E402


@pytest.mark.gpu
def test_forward_spans_and_outputs_as_recorded(tmp_path):
    failed, output, files = mk.run_children(str(tmp_path))      # stops at the first child that exits non-zero
    assert failed is None, f"child {failed}: {output}"
    now = mk.load_device(files)
    with np.load(mk.FIXTURE) as z:
        golden = {k: z[k] for k in mk.DEVICE_KEYS}
    pts = golden["points"].tolist()
    assert now["points"].tolist() == pts and now["kept"].tolist() == golden["kept"].tolist()
    problems = []
    for s, (name, _) in enumerate(mk.SETTINGS):
        bad = np.argwhere((now["spans"][s] != golden["spans"][s]).any(axis=1)).reshape(-1)
        if bad.size:
            i = int(bad[0])
            problems.append(f"{name}: spans differ at {len(bad)} points, first {pts[i]}: {now['spans'][s, i].tolist()} != "
                            f"{golden['spans'][s, i].tolist()} ({mk.KINDS})")
        got, want = now["digests"][now["digest_index"][s]], golden["digests"][golden["digest_index"][s]]
        bad = np.argwhere((got != want).any(axis=1)).reshape(-1)
        if bad.size:
            problems.append(f"{name}: y_out differs at {len(bad)} points, first {pts[int(bad[0])]}")
        for k, i in enumerate(golden["kept"].tolist()):
            y, y0 = now[f"kept_y{k}"][s], golden[f"kept_y{k}"][s]
            diff = np.argwhere(y.view(np.uint32) != y0.view(np.uint32)).reshape(-1)
            if diff.size:
                e = int(diff[0])
                problems.append(f"{name}: kept point {pts[i]}: {len(diff)} of {y.size} elements differ, first y[{e}] = {y[e]!r} != {y0[e]!r}")
    print("\n".join(problems))
    assert not problems, "\n".join(problems[:20])
