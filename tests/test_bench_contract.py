"""The driver's bench.py contract: one JSON line with the agreed keys (checked on the committed round line here,
and on a live run in the GPU tier)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _check_line(j, n_gpus, steps, warmup, with_cpu=True):
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline"):
        assert k in j, k
    assert j["metric"] == "graphs/sec" and j["unit"] == "graphs/s" and j["higher_is_better"] is True
    assert j["n_gpus"] == n_gpus and j["steps"] == steps and j["warmup"] == warmup
    assert j["scaling"] == "weak" and j["data"] == "synthetic" and j["dtype"] == "f32" and j["vs_baseline"] is None
    assert "workload" in j["config"] and "model" not in j["config"]
    # value = graphs of all ranks / max-over-ranks time of the timed steps
    assert abs(j["value"] - j["config"]["global_batch"] / j["ms_per_step"] * 1e3) <= 1e-3 * j["value"]
    r = j["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in r, k
    assert r["bound"] in ("hbm", "mfma") and r["unit"] in ("GB/s", "TFLOP/s")
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-4 and 0 < r["frac"] < 1
    if with_cpu:
        c = j["cpu_baseline"]
        for k in ("value", "unit", "cores", "kind", "sample"):
            assert k in c, k
        assert c["kind"] in ("port", "reference") and c["unit"] == j["unit"] and c["cores"] >= 1 and c["value"] > 0


@pytest.mark.parametrize("name", ["r01_final_bench.json.log", "r02_final_bench.json.log", "r03_final_bench.json.log",
                                  "r04_final_bench.json.log", "r05_final_bench.json.log", "r06_final_bench.json.log"])
def test_committed_round_line_keeps_the_contract(name):
    path = os.path.join(ROOT, "profiles", name)
    if not os.path.exists(path):
        pytest.skip("%s is written at the end of its round" % name)
    lines = [l for l in open(path).read().splitlines() if l.startswith("{")]
    assert len(lines) == 1
    j = json.loads(lines[0])
    _check_line(j, 1, 30, 5)
    if name.startswith("r02"):   # round 2: where the traffic figure comes from, both CPU legs, the other configurations
        assert j["roofline"]["traffic_source"].startswith("profiles/r02_pmc_traffic.json")
        assert j["roofline"]["schedule"] == "dataflow" and "ms_per_step_median" in j
        assert j["cpu_baseline"]["vectorised"]["value"] > 0 and j["cpu_baseline"]["cpu"]
        assert set(j["other_configs"]) >= {"cfg1_NA_B64_h128_L2_unidir", "cfg4_BN_B128_h256_L2_bidir"}
        assert j["training_step"]["ms_per_step_median"] > 0
    if name.startswith("r03"):   # round 3: traffic tied to the kernel sources, one reverse launch, all three other configurations
        assert j["roofline"]["traffic_source"].startswith("profiles/r03_pmc_traffic.json") and j["roofline"]["traffic"] > 0
        assert j["roofline"]["schedule"] == "dataflow" and j["roofline"]["frac"] > 0.15
        assert set(j["other_configs"]) >= {"cfg1_NA_B64_h128_L2_unidir", "cfg4_BN_B128_h256_L2_bidir", "cfg5_code2_B256_h512_L5_bidir"}
        assert j["training_step"]["kernels_ms_per_step"]["backward_run"] < 3.0
    if name.startswith(("r04", "r05", "r06")):   # rounds 4-6: + the reference's own training shape, the full training step with clip_grad_norm
        rnd = name[:3]
        assert j["roofline"]["traffic_source"].startswith("profiles/%s_pmc_traffic.json" % rnd) and j["roofline"]["traffic"] > 0
        assert j["roofline"]["schedule"] == "dataflow" and j["roofline"]["frac"] > 0.18
        assert set(j["other_configs"]) >= {"cfg1_NA_B64_h128_L2_unidir", "cfg4_BN_B128_h256_L2_bidir", "cfg5_code2_B256_h512_L5_bidir",
                                           "ogb_tok_h300_L2_B160"}
        assert j["training_step"]["kernels_ms_per_step"]["backward_run"] < 2.0 and j["training_step"]["ms_per_step_median"] > 0
        assert j["loader_side_plan"]["ms_per_step"] < j["ms_per_step"]
    if name.startswith("r06"):   # round 6: the leaner kernel, the gather stream's own figure, the training tail through the library's entries
        r = j["roofline"]
        assert r["frac"] > 0.22 and r["recurrence_ms_per_forward"] < 1.2
        assert r["gather_GBps"] > 0 and abs(r["gather_frac_of_8TBps"] - r["gather_GBps"] / 8000.0) < 1e-3
        assert r["traffic_split"]["fetch_bytes"] + r["traffic_split"]["write_bytes"] == r["traffic"]
        assert "seq_cross_entropy" in j["training_step"]["loss"] and "ClipAdam" in j["training_step"]["optimizer"]
        h300 = j["other_configs"]["ogb_tok_h300_L2_B160"]["roofline"]
        assert h300["gflop_per_forward"] < h300["gflop_per_forward_padded"]   # priced on the model's own width
    if name.startswith(("r05", "r06")):   # round 5: the line says how the front of the recurrence is built, and times the unfused / unfolded path beside it
        assert "dagnn_prepare" in j["config"]["front_of_recurrence"] and "folded" in j["config"]["front_of_recurrence"]
        assert j["separate_calls_no_folding"]["ms_per_step"] > j["ms_per_step"] > 0
        assert j["kernels_ms_per_step"]["prepare"] < 0.15


def _run_bench(args, env_extra=None, launcher=()):
    env = dict(os.environ)
    env.update(env_extra or {})
    cmd = [sys.executable] + list(launcher) + [os.path.join(ROOT, "bench.py")] + args
    out = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]   # rank 0 prints ONE line
    return json.loads(lines[0])


def test_dump_outputs_keeps_the_cap_and_a_fixed_sample(tmp_path):
    import numpy as np
    import torch
    import bench
    small = [torch.full((4, 3), float(s)) for s in range(2)]
    bench.dump_outputs(small, str(tmp_path / "small"))
    for s in range(2):
        a = np.load(tmp_path / "small" / ("head_%d.npy" % s))
        assert a.dtype == np.float32 and np.array_equal(a, small[s].numpy())
    # 5 heads x 1024 graphs x 5002 vocabulary = 102 MB: a sample of rows, the same rows in every head and on every call
    g = torch.Generator().manual_seed(0)
    big = [torch.randn(1024, 5002, generator=g) for _ in range(5)]
    for t in big:
        t[:, 0] = torch.arange(1024)   # column 0 names the row
    for d in ("a", "b"):
        bench.dump_outputs(big, str(tmp_path / d))
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["head_%d.npy" % s for s in range(5)]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= bench.DUMP_MAX_BYTES
    rows = None
    for s, f in enumerate(files):
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype == np.float32 and a.shape[1] == 5002 and 0 < a.shape[0] < 1024 and np.array_equal(a, b)
        idx = a[:, 0].astype(np.int64)   # which graphs were kept
        assert np.array_equal(a, big[s].numpy()[idx]) and (np.diff(idx) > 0).all() and (rows is None or np.array_equal(idx, rows))
        rows = idx


# what a plain run leaves to `--full`: every figure that takes runs of its own
FULL_ONLY = ("kernels_ms_per_step", "ms_per_step_median", "ms_per_step_p90", "loader_side_plan", "separate_calls_no_folding",
             "two_streams", "strong_scaling", "multi_gpu", "training_step", "other_configs", "cpu_baseline")


def test_full_is_an_option_and_off_by_default():
    import bench
    assert bench.parse_args(["--gpus", "1", "--steps", "3", "--warmup", "1"]).full is False
    a = bench.parse_args(["--gpus", "1", "--steps", "3", "--warmup", "1", "--full"])
    assert a.full is True and (a.steps, a.warmup, a.cpu_passes, a.train_steps, a.other_configs) == (3, 1, 8, 20, 1)


@pytest.mark.gpu
def test_bench_single_gpu_line(tmp_path):
    import numpy as np
    j = _run_bench(["--gpus", "1", "--steps", "3", "--warmup", "1", "--cpu-passes", "0", "--train-steps", "0", "--other-configs", "0",
                    "--dump-outputs", str(tmp_path)])
    _check_line(j, 1, 3, 1, with_cpu=False)
    assert not [k for k in FULL_ONLY if k in j]   # a plain run: the headline and nothing that takes runs of its own
    # the headline forward's five [128, 5002] logit matrices
    for s in range(5):
        a = np.load(tmp_path / ("head_%d.npy" % s))
        assert a.dtype == np.float32 and a.shape == (128, 5002) and np.isfinite(a).all()


@pytest.mark.gpu
def test_bench_full_adds_the_further_legs():
    """`--full` with the long legs sized down (two training steps, no CPU baseline, no other configurations): the same
    headline keys, plus the second pass, the three forward variants and the training step."""
    j = _run_bench(["--gpus", "1", "--steps", "3", "--warmup", "1", "--full", "--cpu-passes", "0", "--train-steps", "2",
                    "--other-configs", "0"])
    _check_line(j, 1, 3, 1, with_cpu=False)
    assert j["kernels_ms_per_step"]["prepare"] > 0 and j["ms_per_step_p90"] >= j["ms_per_step_median"] > 0
    for k in ("loader_side_plan", "separate_calls_no_folding", "two_streams"):
        assert j[k]["ms_per_step"] > 0 and j[k]["graphs_per_s"] > 0, k
    t = j["training_step"]
    assert t["steps"] == 2 and t["ms_per_step"] > 0 and t["kernels_ms_per_step"]["backward_run"] > 0
    assert "cpu_baseline" not in j and "other_configs" not in j


@pytest.mark.gpu
def test_bench_two_ranks_under_torchrun():
    """The driver's N > 1 launch line (`python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N`);
    here two ranks share the one visible GPU and rendezvous over gloo (RCCL refuses two ranks on one device)."""
    launcher = ["-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                "--master-port", "29517"]
    j = _run_bench(["--gpus", "2", "--steps", "3", "--warmup", "1", "--full", "--cpu-passes", "0", "--train-steps", "2",
                    "--other-configs", "0"],
                   env_extra={"DAGNN_BENCH_BACKEND": "gloo"}, launcher=launcher)
    _check_line(j, 2, 3, 1, with_cpu=False)
    assert j["config"]["global_batch"] == 256   # weak scaling: 128 graphs per rank
    # the line explains itself at N > 1: per-rank group counts / reserved CUs, the rank-seeds weak-scaling entry, the strong-scaling leg
    m = j["multi_gpu"]
    assert [r["rank"] for r in m["per_rank"]] == [0, 1]
    assert all(r["dataflow_groups_inference"] >= r["dataflow_groups_training"] > 0 and r["reserved_cus_training"] in (0, 64)
               for r in m["per_rank"])
    w = m["weak_scaling_rank_seeds"]
    assert w["graphs_per_s"] > 0 and len(w["nodes_layers_per_rank"]) == 2 and w["nodes_layers_per_rank"][0] != w["nodes_layers_per_rank"][1]
    assert j["strong_scaling"]["scaling"] == "strong" and "allreduce_exposed_ms" in j["training_step"]
