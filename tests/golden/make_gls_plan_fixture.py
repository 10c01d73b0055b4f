"""Regenerates tests/golden/gls_plan_grid.npz: what the host-side launch queries of the C ABI answer over a grid of
(n, B, penalty_bits, first_improvement) and the three experiment overrides (team mode, prune mode, forced thread count).

    python tests/golden/make_gls_plan_fixture.py        (CPU only: without a GPU the library counts 256 CUs, the MI355X's)

Recorded at the commit named in the file (`commit`), before the launch policy moved into csrc/gls_plan.cpp; test_gls_plan_cpu.py
replays the grid and requires equality at every point.  Arrays only, narrowest integer dtype each:
  n, B, penalty_bits            the default-override grid (axes of the `d_*` arrays, then first_improvement 0 / 1)
  sub_n, configs                the override grid: `o_*` arrays have the axes (config, sub_n, B, penalty_bits, first_improvement),
                                a config is (team mode, prune mode, thread override)
  *_run_rc, *_run_<field>       gnngls_gls_describe_run: return code and its seven outputs (-1 where the call left them alone)
  *_cfg_rc, *_cfg_<field>       gnngls_gls_describe_config (no first_improvement axis): return code and its four outputs
  *_wps, *_team                 gnngls_gls_waves_per_simd, gnngls_gls_uses_team (no first_improvement axis)
  *_capacity, *_chunk           gnngls_gls_resident_capacity(n), gnngls_regret_labels_chunk(n) (axes: [config,] n)"""
import ctypes
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
GOLDEN = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(GOLDEN, "gls_plan_grid.npz")

N = list(range(3, 261)) + [300, 400, 1000, 5000, 70000]
B = [0, 1, 8, 128, 256, 257, 512, 513, 625, 700, 1000, 1024, 1025, 1250, 1536, 2048, 2049, 3000, 4096, 4097, 5000, 8192]
BITS = [0, 16, 32, -1, -2, 7]
SUB_N = [7, 8, 20, 24, 25, 30, 33, 34, 48, 49, 50, 63, 64, 80, 81, 100, 127, 128, 143, 144, 150, 163, 164, 200, 255, 256]
CONFIGS = [(0, -1, 0), (1, -1, 0), (-1, 0, 0), (-1, -1, 64), (-1, -1, 128), (-1, -1, 256), (-1, -1, 512)]
RUN_FIELDS = [("store", np.int16), ("threads", np.int16), ("lds", np.int32), ("per_cu", np.int8), ("wps", np.int8),
              ("team", np.int8), ("edge", np.int8)]
CFG_FIELDS = RUN_FIELDS[:4]


def set_overrides(L, team=-1, prune=-1, threads=0):
    assert L.gnngls_debug_set_gls_team(team) == 0 and L.gnngls_debug_set_gls_prune(prune) == 0
    assert L.gnngls_debug_set_gls_threads(threads) == 0


def sweep(L, ns, prefix):
    """-> dict of arrays over (ns, B, BITS[, first_improvement]) under the overrides currently set."""
    shape = (len(ns), len(B), len(BITS))
    out = {prefix + "run_rc": np.zeros(shape + (2,), np.int8), prefix + "cfg_rc": np.zeros(shape, np.int8),
           prefix + "wps": np.zeros(shape, np.int8), prefix + "team": np.zeros(shape, np.int8),
           prefix + "capacity": np.zeros(len(ns), np.int32), prefix + "chunk": np.zeros(len(ns), np.int32)}
    for name, dt in RUN_FIELDS:
        out[prefix + "run_" + name] = np.zeros(shape + (2,), dt)
    for name, dt in CFG_FIELDS:
        out[prefix + "cfg_" + name] = np.zeros(shape, dt)
    vals = [ctypes.c_int(0) for _ in range(7)]
    ptrs = [ctypes.cast(ctypes.byref(v), ctypes.c_void_p) for v in vals]
    for i, n in enumerate(ns):
        out[prefix + "capacity"][i] = L.gnngls_gls_resident_capacity(n)
        out[prefix + "chunk"][i] = L.gnngls_regret_labels_chunk(n)
        for j, b in enumerate(B):
            for k, bits in enumerate(BITS):
                for fi in (0, 1):
                    for v in vals:
                        v.value = -1
                    out[prefix + "run_rc"][i, j, k, fi] = L.gnngls_gls_describe_run(n, b, bits, fi, *ptrs)
                    for (name, _), v in zip(RUN_FIELDS, vals):
                        out[prefix + "run_" + name][i, j, k, fi] = v.value
                for v in vals:
                    v.value = -1
                out[prefix + "cfg_rc"][i, j, k] = L.gnngls_gls_describe_config(n, b, bits, *ptrs[:4])
                for (name, _), v in zip(CFG_FIELDS, vals):
                    out[prefix + "cfg_" + name][i, j, k] = v.value
                out[prefix + "wps"][i, j, k] = L.gnngls_gls_waves_per_simd(n, b, bits)
                out[prefix + "team"][i, j, k] = L.gnngls_gls_uses_team(n, b, bits)
    return out


def record(L):
    """The whole grid on the loaded library -> dict of arrays (the fixture without its `commit`)."""
    out = {"n": np.asarray(N, np.int32), "B": np.asarray(B, np.int16), "penalty_bits": np.asarray(BITS, np.int8),
           "sub_n": np.asarray(SUB_N, np.int16), "configs": np.asarray(CONFIGS, np.int16)}
    try:
        set_overrides(L)
        out.update(sweep(L, N, "d_"))
        per_config = []
        for team, prune, threads in CONFIGS:
            set_overrides(L, team, prune, threads)
            per_config.append(sweep(L, SUB_N, "o_"))
        for key in per_config[0]:
            out[key] = np.stack([p[key] for p in per_config])
    finally:
        set_overrides(L)
    return out


def main():
    from gnngls_amd import _lib, build
    build.build()
    arrays = record(_lib.load())
    commit = subprocess.check_output(["git", "rev-parse", "HEAD"], cwd=ROOT).decode().strip()
    np.savez_compressed(FIXTURE, commit=np.asarray(commit), **arrays)
    print(os.path.basename(FIXTURE), os.path.getsize(FIXTURE), "bytes,", commit)


if __name__ == "__main__":
    main()
