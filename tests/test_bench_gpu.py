"""GPU smoke tests of bench.py itself: the single-rank line and the multi-rank path (2 ranks sharing one GPU over
gloo -- the only difference to the driver's torchrun launch is the backend of the final gather)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def last_json_line(out):
    lines = [l for l in out.decode().splitlines() if l.startswith("{")]
    assert lines, out.decode()[-2000:]
    return json.loads(lines[-1])


def test_bench_single_rank_small(tmp_path):
    # (one warm-up step: the first forward pass of a process loads the code objects, which would eat the 0.5 s budget)
    out = subprocess.check_output([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "1", "--warmup", "1",
                                   "--batch", "64", "--time_limit", "0.5", "--cpu_cores", "8", "--no_gap_bracket",
                                   "--dump-outputs", str(tmp_path / "dump")], cwd=ROOT, stderr=subprocess.STDOUT, timeout=600)
    j = last_json_line(out)
    # --dump-outputs: the arrays the timed step returned, the numbers of the line among them
    d = {f[:-4]: np.load(os.path.join(tmp_path, "dump", f)) for f in os.listdir(tmp_path / "dump")}
    assert d["best_cost"].shape == (64,) and d["best_tour"].shape == (64, 101) and d["regret_pred"].shape == (64, 100, 100)
    assert all(a.dtype in (np.float32, np.float64) for a in d.values()) and "sample_index" not in d
    assert abs(d["best_cost"].mean() - j["mean_best_cost"]) < 1e-9 and abs(d["init_cost"].mean() - j["mean_init_cost"]) < 1e-9
    assert (d["best_cost"] <= d["init_cost"]).all() and (np.sort(d["best_tour"][:, :-1], axis=1) == np.arange(100)).all()
    assert j["n_gpus"] == 1 and j["steps"] == 1 and j["warmup"] == 1 and j["unit"] == "instances/s"
    assert 64 / 1.5 < j["value"] < 64 / 0.45
    r = j["roofline"]
    # round 6: the fraction is SURVEY 8(d)'s executed-LDS figure, measured in the run or withheld -- never borrowed.  64 instances run on
    # the LDS-penalty store, which prunes (n = 100) but has no counting instantiation: the line says so instead of guessing
    assert r["kernel"] == "gls_kernel" and r["bound"] == "lds" and "SURVEY 8(d)" in r["frac_definition"] and r["frac"] is None
    assert r["reference_equivalent_evals_per_s"] > 0 and r["prune_ratio"] is None and r["executed_evals_per_s"] is None
    assert 0 < r["reference_equivalent_frac"] < 1.5
    # the committed counters are the headline's (TSP100 x 1024): not this workload's, so no pipes / traffic are derived from them
    assert not r["pmc_matches_workload"] and r["pmc"] is None and r["busiest_pipes"] is None and r["traffic"] is None
    assert r["critical_path"] is None                       # no counting instantiation, no cycle records
    assert r["launches"] == 1 and j["config"]["rounds_per_rank"] == [1]
    # search-progress record of the timed step: the gap never rises with the budget, its end point is the headline gap
    c = j["gap_vs_budget"]
    assert [p["t_s"] for p in c[:-1]] == [0.1, 0.3] and 0.3 < c[-1]["t_s"] < 0.5      # grid points inside the 0.5 s budget + its end
    assert all(a["mean_gap_pct"] >= b["mean_gap_pct"] - 1e-12 for a, b in zip(c, c[1:]))
    assert all(a["at_best_known_pct"] <= b["at_best_known_pct"] + 1e-12 for a, b in zip(c, c[1:]))
    assert abs(c[-1]["mean_gap_pct"] - j["mean_gap_pct"]) < 1e-9 and abs(c[-1]["budget_t_s"] - 0.5) < 1e-6
    assert j["improvement_trace_truncated_instances"] == 0
    # iso-quality pass: 10 device loads of 64 instances inside ONE 0.5 s limit
    q = j["iso_quality"]
    assert q["rounds"] == 10 and q["instances"] == 640 and q["budget"] == "per_batch"
    assert 640 / 1.6 < q["instances_per_s"] < 640 / 0.45 and q["mean_gap_pct"] >= j["mean_gap_pct"] - 1e-9
    f = q["frontier"]                                        # the same loads inside the full limit, a third and a tenth of it
    assert [round(p["time_limit_s"], 6) for p in f] == [0.5, round(0.5 / 3, 6), 0.05] and f[0]["instances_per_s"] == q["instances_per_s"]
    assert all(0 < p["forward_share"] <= 1.2 and p["instances"] == 640 for p in f) and f[2]["instances_per_s"] > f[0]["instances_per_s"]
    assert j["config"]["residency_utilisation"] == [64 / 1024] and j["config"]["backend"] is None
    w = j["cpu_baseline"]["whole_box_estimate"]
    assert w["physical_cores"] >= 1 and w["instances_per_s"] > 0 and w["gpu_over_whole_box"] > 0
    assert [p["t_s"] for p in j["cpu_baseline"]["gap_vs_budget"]] == [0.1, 0.3, 0.5]
    assert all(k["bound"] in ("hbm", "mfma") for k in j["kernels"].values()) and "ffn_fused" in j["kernels"]
    assert j["cpu_baseline"]["cores"] == 8 and j["cpu_baseline"]["kind"] == "port"
    assert j["watchdog_aborts"] == 0
    # gap against the committed best-known file (independent of this run); a 0.5 s search stays above it
    assert "bench_data/" in j["gap_reference"] and j["mean_gap_pct"] >= 0 and j["instances_below_reference"] == 0


def test_bench_one_rank_through_rccl():
    """backend "nccl" (= RCCL) with a process group of ONE rank: the torchrun launch of the driver, device-side gather,
    barrier, all_reduce(MAX) and all_gather of the N-rank path all execute on RCCL -- what a one-GPU box can run of it."""
    env = dict(os.environ, GNNGLS_DIST_SINGLE="1")
    env.pop("GNNGLS_DIST_BACKEND", None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
           "--master-port", "29532", os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "1", "--warmup", "1",
           "--batch", "640", "--time_limit", "0.5", "--no_cpu_baseline", "--no_gap_bracket", "--no_iso_quality"]
    out = subprocess.check_output(cmd, cwd=ROOT, env=env, stderr=subprocess.STDOUT, timeout=600)
    j = last_json_line(out)
    assert j["n_gpus"] == 1 and 640 / 1.5 < j["value"] < 640 / 0.45 and j["watchdog_aborts"] == 0
    # 640 TSP100 instances run on the compact store (the headline's): the counting pass reports what the pruned 2-opt scan saves
    r = j["roofline"]
    assert 0 < r["prune_ratio"] < 1 and abs(r["executed_evals_per_s"] - r["prune_ratio"] * r["reference_equivalent_evals_per_s"]) < 1e-3 * r["executed_evals_per_s"]
    assert r["bound"] == "lds" and 0 < r["frac"] < r["reference_equivalent_frac"] < 1.5 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-12
    assert j["config"]["rounds_per_rank"] == [1] and len(j["gls_ms_per_rank"]) == 1 and j["mean_gap_pct"] >= 0
    assert j["config"]["backend"] == "RCCL (nccl)" and "RCCL" in j["config"]["parallelism"] and j["config"]["world_size"] == 1
    assert j["config"]["collectives_per_step"] == {"gather": 1.0}


def test_bench_two_ranks_gloo():
    env = dict(os.environ, GNNGLS_DIST_BACKEND="gloo")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29533", os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "1",
           "--batch", "64", "--time_limit", "0.5", "--no_gap_bracket"]
    out = subprocess.check_output(cmd, cwd=ROOT, env=env, stderr=subprocess.STDOUT, timeout=600)
    j = last_json_line(out)
    assert j["n_gpus"] == 2 and j["scaling"] == "weak"
    assert j["config"]["backend"] == "gloo" and "gloo" in j["config"]["parallelism"] and "RCCL" not in j["config"]["parallelism"]
    assert j["config"]["collectives_per_step"] == {"gather": 1.0} and "iso_quality" not in j
    assert len(j["gap_vs_budget"]) == 3 and abs(j["gap_vs_budget"][-1]["mean_gap_pct"] - j["mean_gap_pct"]) < 1e-9
    assert 128 / 2.5 < j["value"] < 128 / 0.45          # whole-job aggregate over both ranks
    assert "cpu_baseline" not in j                      # rank 0, N=1 only
    assert j["config"]["rounds_per_rank"] == [1, 1] and len(j["gls_ms_per_rank"]) == 2


def test_bench_strong_scaling_two_ranks_gloo():
    """--total_instances: a FIXED test set cut into contiguous shards (BASELINE configs[3] in miniature: 151 TSP20
    instances over 2 ranks = shards of 76 and 75; with a residency of 32 every rank needs 3 rounds of the full budget),
    uneven shards, one gather."""
    env = dict(os.environ, GNNGLS_DIST_BACKEND="gloo")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29534", os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0",
           "--tsp_n", "20", "--total_instances", "151", "--time_limit", "0.4", "--guides", "weight", "--resident_instances", "32"]
    out = subprocess.check_output(cmd, cwd=ROOT, env=env, stderr=subprocess.STDOUT, timeout=600)
    j = last_json_line(out)
    assert j["n_gpus"] == 2 and j["scaling"] == "strong" and j["config"]["total_instances"] == 151
    assert j["config"]["rounds_per_rank"] == [3, 3]
    assert 151 / 4.0 < j["value"] < 151 / 1.15          # 3 rounds x 0.4 s
    assert j["mean_gap_pct"] is None and "no best-known file" in j["gap_reference"]       # TSP20 has no committed file


def run_ranks(nproc, port, extra, timeout=900):
    env = dict(os.environ, GNNGLS_DIST_BACKEND="gloo")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", str(nproc), "--steps", "1", "--warmup", "0",
           "--no_gap_bracket"] + extra
    return last_json_line(subprocess.check_output(cmd, cwd=ROOT, env=env, stderr=subprocess.STDOUT, timeout=timeout))


def test_bench_four_ranks_configs3_in_miniature():
    """The driver's multi-GPU launch of BASELINE configs[3] (a fixed test set cut into contiguous shards, test.py:59), rehearsed
    with 4 ranks sharing the one GPU over gloo (not 8: with the test process that would be more than six processes holding the
    one device): 501 TSP20 instances -> shards of 126 x 3 + 123, two rounds of the full budget per rank at a residency of 64,
    ONE gather per step, every rank bound to device local_rank % visible devices."""
    j = run_ranks(4, 29541, ["--tsp_n", "20", "--total_instances", "501", "--time_limit", "0.3", "--guides", "weight",
                             "--resident_instances", "64"])
    c = j["config"]
    assert j["n_gpus"] == 4 and j["scaling"] == "strong" and c["total_instances"] == 501 and c["world_size"] == 4
    assert c["rounds_per_rank"] == [2] * 4 and c["collectives_per_step"] == {"gather": 1.0} and c["backend"] == "gloo"
    assert c["device_of_rank"] == [r % c["visible_devices"] for r in range(4)]
    util = c["residency_utilisation"]
    assert all(abs(u - 126 / 128) < 1e-12 for u in util[:3]) and abs(util[3] - 123 / 128) < 1e-12
    assert 501 / 3.0 < j["value"] < 501 / 0.6 and j["watchdog_aborts"] == 0      # 2 rounds x 0.3 s, four ranks on one GPU
    assert len(j["gls_ms_per_rank"]) == 4 and j["roofline"]["launches"] == 2


def test_bench_four_ranks_configs4_in_miniature():
    """BASELINE configs[4] per GPU (TSP200, weak scaling: rank r searches its own block, one round) with 4 ranks on the one
    GPU: 4 instances per rank, the 16-wave compact-store workgroups of TSP200."""
    j = run_ranks(4, 29542, ["--tsp_n", "200", "--batch", "4", "--time_limit", "0.5", "--guides", "weight"])
    c = j["config"]
    assert j["n_gpus"] == 4 and j["scaling"] == "weak" and c["total_instances"] == 16 and c["instances_per_gpu"] == 4
    assert c["rounds_per_rank"] == [1] * 4 and c["collectives_per_step"] == {"gather": 1.0}
    assert 16 / 2.5 < j["value"] < 16 / 0.45 and j["watchdog_aborts"] == 0 and j["outer_iters_per_instance"] > 10
