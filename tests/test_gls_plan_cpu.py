"""The launch plan of the search kernel (csrc/gls_plan.cpp) decides what it decided before it was one function:
tests/golden/gls_plan_grid.npz holds what the host-side queries of the C ABI answered, over a grid of shapes and experiment
overrides, at the commit named in the file (tests/golden/make_gls_plan_fixture.py).

* the C ABI of the library as built now answers the same at every point;
* the plan unit alone -- plain C++, compiled here with the host compiler under AddressSanitizer + UndefinedBehaviorSanitizer
  into tests/gls_plan_sweep.cpp, a process of its own -- sweeps the same grid with the trace and the executed-evaluation
  count asked for and not, exits clean, and reports the same seven gnngls_gls_describe_run fields."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import make_gls_plan_fixture as mk  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    with np.load(mk.FIXTURE) as z:
        g = {k: z[k] for k in z.files}
    assert g["n"].tolist() == mk.N and g["B"].tolist() == mk.B and g["penalty_bits"].tolist() == mk.BITS
    assert g["sub_n"].tolist() == mk.SUB_N and g["configs"].tolist() == [list(c) for c in mk.CONFIGS]
    return g


def test_fixture_covers_every_kind_of_plan(golden):
    """The grid reaches every store, workgroup size, register budget and both forms of the perturbation phase."""
    ok = golden["d_run_rc"] == 0
    assert set(np.unique(golden["d_run_store"][ok])) == {0, 116, 132, 200}
    assert set(np.unique(golden["d_run_threads"][ok])) == {64, 128, 256, 512, 1024}
    assert set(np.unique(golden["d_run_wps"][ok])) == {2, 4, 6, 8}
    assert set(np.unique(golden["d_run_team"][ok])) == {0, 1} and set(np.unique(golden["d_run_edge"][ok])) == {0, 1}
    assert set(np.unique(golden["d_run_rc"])) == {0, -1, -3}            # GNNGLS_ERR_ARG (penalty_bits 7), _UNSUPPORTED (LDS)
    forced = golden["o_run_team"] == 1                                  # override configs: team mode 0, team mode 1, ...
    assert golden["configs"][:2, 0].tolist() == [0, 1] and not forced[0].any() and forced[1].any()


def test_c_abi_queries_answer_as_recorded(golden):
    from gnngls_amd import _lib, build
    build.build()
    now = mk.record(_lib.load())
    assert sorted(now) == sorted(k for k in golden if k != "commit")
    for key, want in golden.items():
        if key == "commit":
            continue
        got = now[key]
        assert got.dtype == want.dtype and got.shape == want.shape, key
        bad = np.argwhere(got != want)
        assert bad.size == 0, f"{key}: {len(bad)} points differ, first at index {bad[0].tolist()}: {got[tuple(bad[0])]} != {want[tuple(bad[0])]}"


def test_plan_unit_alone_under_asan_ubsan(golden, tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++")
    assert cxx, "no host C++ compiler"
    exe, grid = str(tmp_path / "gls_plan_sweep"), str(tmp_path / "grid.txt")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "gls_plan_sweep.cpp"),
                           os.path.join(ROOT, "gnngls_amd", "csrc", "gls_plan.cpp"), "-o", exe])
    with open(grid, "w") as f:
        for row in (golden["n"], golden["B"], golden["penalty_bits"], golden["sub_n"], golden["configs"].ravel()):
            f.write(" ".join(str(int(v)) for v in row) + "\n")
    out = subprocess.run([exe, grid], capture_output=True, timeout=600)
    assert out.returncode == 0 and not out.stderr, out.stderr.decode()[-3000:]
    rec = np.frombuffer(out.stdout, dtype=np.int32).reshape(-1, 7)
    fields = [name for name, _ in mk.RUN_FIELDS]
    want = np.concatenate([np.stack([golden[p + "run_" + f].astype(np.int32).reshape(-1) for f in fields], axis=1)
                           for p in ("d_", "o_")])
    rc = np.concatenate([golden["d_run_rc"].reshape(-1), golden["o_run_rc"].reshape(-1)])
    assert rec.shape == want.shape
    # (where the C ABI refused the arguments it left its outputs alone: nothing to compare there)
    bad = np.argwhere((rec != want).any(axis=1) & (rc == 0))
    assert bad.size == 0, f"{len(bad)} points differ, first record {int(bad[0])}: {rec[int(bad[0])].tolist()} != {want[int(bad[0])].tolist()}"
