"""The regret forward's plan (csrc/model_plan.cpp) decides what the forward decided before it was one function:
tests/golden/forward_plan_grid.npz holds what the C ABI answered and what the forward launched and computed on an MI355X, over the
smallest shapes at which each decision can flip, at the commit named in the file (tests/golden/make_forward_plan_fixture.py).

* the fixture reaches every kind of plan;
* the C ABI of the library as built now answers the host part -- sizes, return codes, error texts -- as recorded;
* the plan unit alone -- plain C++, compiled here with the host compiler under AddressSanitizer + UndefinedBehaviorSanitizer into
  tests/forward_plan_sweep.cpp, a process of its own -- sweeps the whole grid under the four switch settings, exits clean, and its
  step lists imply the recorded profile spans at every accepted point and the recorded return code at every refused one."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import make_forward_plan_fixture as mk  # noqa: E402

HOST_KEYS = ["size_n", "size_B", "size_heads", "size_layers", "size_in_dims", "pf_floats", "pb_bytes", "fw_bytes", "fw_bytes_heads",
             "tw_bytes", "tw_bytes_heads", "ref_call", "ref_rc", "ref_text"]


@pytest.fixture(scope="module")
def golden():
    with np.load(mk.FIXTURE) as z:
        g = {k: z[k] for k in z.files}
    assert sorted(g) == sorted(["commit"] + HOST_KEYS + mk.DEVICE_KEYS)
    assert len(str(g["commit"])) == 40
    assert g["points"].tolist() == [list(p) for p in mk.accepted_points()]
    assert g["settings"].tolist() == [name for name, _ in mk.SETTINGS]
    assert g["ref_call"].tolist() == [c[0] for c in mk.refused_calls()]
    assert g["spans"].shape == (len(mk.SETTINGS), len(g["points"]), len(mk.KINDS)) and g["digests"].shape[1] == 32
    return g


def test_fixture_covers_every_kind_of_plan(golden):
    spans = golden["spans"].reshape(-1, len(mk.KINDS)).astype(int)
    embed, fc, gat, rank1, ffn, dec = spans.T
    layers = np.tile(golden["points"][:, 2].astype(int), len(mk.SETTINGS))
    chunks = np.maximum(embed, np.maximum(ffn // np.maximum(layers, 1), dec))
    assert (embed == 0).any()                                       # no embedding pass at all
    assert (rank1 > 0).any() and ((rank1 > 0) & (embed > 0)).any()  # the rank-1 first GATConv, compact and with h_0 kept
    assert (dec > 0).any() and (dec == 0).any()                     # a decision launch of its own, and folded into the feed-forward
    assert ((layers == 3) & (fc == 3 * chunks)).any() and ((layers == 3) & (fc == chunks)).any() and ((layers > 0) & (fc == 0)).any()
    assert (chunks == 2).any() and (chunks == 1).any()              # a chunked forward
    assert ((gat + rank1 == ffn) & (ffn == layers * chunks)).all()
    assert set(golden["ref_rc"].tolist()) == {mk.ERR_ARG, mk.ERR_UNSUPPORTED}           # both refusal codes
    large = golden["points"][:, 0] >= 116
    assert large.any() and (golden["points"][large, 5] == 0).all() and (golden["points"][large, 2] == 1).all()
    # the switch settings change what runs, and what comes out, somewhere
    assert all((golden["spans"][0] != golden["spans"][k]).any() for k in (1, 2, 3))
    assert all((golden["digest_index"][0] != golden["digest_index"][k]).any() for k in (1, 2))
    assert np.isfinite(np.concatenate([golden[f"kept_y{k}"].reshape(-1) for k in range(len(mk.KEPT))])).all()


def test_c_abi_answers_the_host_part_as_recorded(golden):
    from gnngls_amd import _lib, build
    build.build()
    now = mk.record_host(_lib.load())
    assert sorted(now) == sorted(HOST_KEYS)
    for key in HOST_KEYS:
        got, want = now[key], golden[key]
        assert got.dtype == want.dtype and got.shape == want.shape, key
        bad = np.argwhere(got != want)
        where = golden["ref_call"][bad[0][0]] if bad.size and key.startswith("ref_") else ""
        assert bad.size == 0, f"{key}: {len(bad)} points differ, first at index {bad[0].tolist()} {where}: {got[tuple(bad[0])]!r} != {want[tuple(bad[0])]!r}"


def test_plan_unit_alone_under_asan_ubsan(golden, tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++")
    assert cxx, "no host C++ compiler"
    exe, grid = str(tmp_path / "forward_plan_sweep"), str(tmp_path / "grid.txt")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "forward_plan_sweep.cpp"),
                           os.path.join(ROOT, "gnngls_amd", "csrc", "model_plan.cpp"), "-o", exe])
    # what the recorded runs were given, from the recorded sizes: the workspace of bmode 0 / 1 / 2 holds 1 / 2 / 3 instances and
    # bmode 2 loses 252 bytes to the alignment
    ni = {n: i for i, n in enumerate(golden["size_n"].tolist())}
    hi = {h: i for i, h in enumerate(golden["size_heads"].tolist())}
    li = {v: i for i, v in enumerate(golden["size_layers"].tolist())}
    di = {v: i for i, v in enumerate(golden["size_in_dims"].tolist())}
    sized_for = golden["size_B"].tolist()
    pts = mk.grid_points()
    with open(grid, "w") as f:
        for n, H, layers, in_dim, form, bmode in pts:
            avail = int(golden["fw_bytes_heads"][sized_for.index(bmode + 1), ni[n], hi[H]]) - (252 if bmode == 2 else 0)
            f.write(f"{n} {H} {layers} {in_dim} {form} {mk.batch_of(bmode)} {avail} {int(golden['pb_bytes'][li[layers]])} "
                    f"{int(golden['pf_floats'][di[in_dim], li[layers]])}\n")
    out = subprocess.run([exe, grid], capture_output=True, timeout=600)
    assert out.returncode == 0 and not out.stderr, out.stderr.decode()[-3000:]
    rec = np.frombuffer(out.stdout, dtype=np.int32).reshape(len(mk.SETTINGS), len(pts), 8)
    row_of = {tuple(p): i for i, p in enumerate(golden["points"].tolist())}
    refused = dict(zip(golden["ref_call"].tolist(), golden["ref_rc"].tolist()))
    n_refused = 0
    for s, (name, _) in enumerate(mk.SETTINGS):
        for i, p in enumerate(pts):
            status, Bc, spans = int(rec[s, i, 0]), int(rec[s, i, 1]), rec[s, i, 2:].tolist()
            if p in row_of:
                want = golden["spans"][s, row_of[p]].tolist()
                assert status == 0 and spans == want, f"{name} {p}: status {status}, spans {spans} != {want}"
                assert Bc == (2 if p[5] == 1 else mk.batch_of(p[5])), f"{name} {p}: Bc {Bc}"
            else:
                n_refused += 1
                assert status == refused[mk.grid_refusal_desc(p)] and status != 0 and Bc == 0, f"{name} {p}: status {status}"
    assert n_refused == len(mk.SETTINGS) * (len(pts) - len(row_of)) > 0
