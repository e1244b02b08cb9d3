"""bench.py --gpus N on CPU: the launcher starts N ranks (one process per GPU, distinct
LOCAL_RANK = device) when no launcher set WORLD_SIZE, relays rank 0's JSON line, and
reports the N > 1 run as the driver reads it -- with tests/bench_stub.py standing in for
the per-GPU sampler (no kernel; each launch sleeps a known time).  Reference: the
launch-sized world of ``mpiexec -n W python apf_step2.py`` (apf_step2.py:27-29, :50-57)."""
import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(REPO, "tests")
WPG, ITERS, STRIDE, STEPS = 64, 100, 10, 3


def _run(args, extra_env=None, timeout=180):
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT",
                        "TORCHELASTIC_RUN_ID", "OLPE_BENCH_LAUNCHED")}
    env.update(OLPE_BENCH_SAMPLER="bench_stub:StubSampler", OLPE_STUB_MS="20",
               PYTHONPATH=os.pathsep.join([TESTS, REPO, env.get("PYTHONPATH", "")]))
    env.update(extra_env or {})
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--walkers", str(WPG),
           "--steps", str(STEPS), "--warmup", "1", "--no-cpu-baseline", "--no-alt"] + args
    return subprocess.run(cmd, cwd=REPO, env=env, capture_output=True, text=True,
                          timeout=timeout)


def _line(r):
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, (r.stdout, r.stderr)
    return json.loads(lines[0])


@pytest.mark.parametrize("n", [2, 8])
def test_gpus_flag_spawns_n_ranks(n):
    r = _run(["--gpus", str(n)])
    assert r.returncode == 0, r.stderr
    d = _line(r)
    assert d["n_gpus"] == n
    c = d["config"]
    assert c["parallelism"] == f"walker-sharded x{n}"
    assert c["launcher"] == "bench.py --gpus"
    assert c["local_ranks"] == list(range(n)) and c["devices"] == list(range(n))
    # value = every rank's walker-steps / the max-over-ranks wall time of the timed steps
    total = n * WPG * ITERS * STEPS
    assert d["value"] == pytest.approx(total / (d["ms_per_step"] * STEPS * 1e-3), rel=1e-9)
    assert d["ms_per_step"] >= 20.0                        # each stub launch sleeps 20 ms
    # the exchange: state all-gather checked against this rank's block, then the chain
    # concatenation over every rank's rows
    nrec, ps = ITERS // STRIDE, 17
    assert d["allgather_ms"] is not None and "comm_error" not in d
    assert d["chain_gather_bytes"] == n * WPG * nrec * ps * 8
    assert d["chain_gather_ranges"] == 1 and d["chain_gather_range_walkers"] == WPG
    assert d["chain_gather_gbs"] == pytest.approx(
        d["chain_gather_bytes"] * (n - 1) / n / (d["chain_gather_ms"] * 1e-3) / 1e9, rel=1e-9)
    # posterior over every rank's walkers (the all-reduced moments)
    assert d["posterior"]["walkers"] == n * WPG
    # RCCL's own view of the communicator on every rank, and the walker total the
    # moments all-reduce summed (verdict r05 item 1)
    drill = d["comm"].pop("fault_drill")
    assert d["comm"] == {"rccl_nranks": n, "rccl_ranks": list(range(n)),
                         "rccl_nranks_agree": True, "walkers_allreduced": n * WPG}
    # the fault drill after the exchange: a fault on one rank is an error on every rank,
    # and the next call recovers the summary everywhere
    assert drill["ok"] is True and len(drill["cases"]) == 2
    for case, who in zip(drill["cases"], (n - 1, 0)):
        assert case["rank"] == who and case["recovered"] is True
        assert case["codes"] == [-2 if r == who else -5 for r in range(n)]
    assert d["posterior"]["rows_per_walker"] == (STEPS + 1) * nrec
    assert "cpu_baseline" not in d                     # rank 0 at N = 1 only
    # stdout is the JSON line alone: the communicator's banner went to stderr
    assert [ln for ln in r.stdout.splitlines() if ln.strip()] == [r.stdout.strip()]
    assert "RCCL version : stub banner" in r.stderr


def test_chain_gather_ranges_and_verify():
    # 64 walkers x 10 rows x 136 B = 87,040 B per rank; a 0.02 MiB range holds 15 walkers
    r = _run(["--gpus", "2", "--gather-mib", "0.02", "--verify-exchange"])
    assert r.returncode == 0, r.stderr
    d = _line(r)
    wn = int(0.02 * 2 ** 20 // (10 * 17 * 8))
    assert d["chain_gather_range_walkers"] == wn
    assert d["chain_gather_ranges"] == -(-WPG // wn)
    assert d["exchange_verified"] is True


def test_exchange_error_is_reported_in_the_line():
    r = _run(["--gpus", "2"], {"OLPE_STUB_FAIL": "chain"})
    assert r.returncode == 0, r.stderr
    d = _line(r)
    assert "injected failure" in d["comm_error"]
    assert d["n_gpus"] == 2 and d["value"] > 0            # the measurement survives


def test_failed_rank_fails_the_launch():
    r = _run(["--gpus", "3"], {"OLPE_STUB_FAIL": "rank1"}, timeout=120)
    assert r.returncode != 0
    assert "rank 1 exited with status 5" in r.stderr
    assert not [ln for ln in r.stdout.splitlines() if ln.startswith("{")]


def test_world_size_mismatch_is_refused():
    r = _run(["--gpus", "3"], {"WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode == 2
    assert "WORLD_SIZE=2" in r.stderr


def test_one_rank_without_launcher():
    r = _run([])
    assert r.returncode == 0, r.stderr
    d = _line(r)
    assert d["n_gpus"] == 1 and d["config"]["launcher"] == "none (1 rank)"
    assert d["config"]["devices"] == [0] and d["allgather_ms"] is None


def test_config0_line_beside_one_core():
    """configs[0] (1 walker, 32x32, 1,000 iterations): the GPU's one walker beside the
    oracle's one walker on one core, and the reference's own rate derived from the
    build-container ratio (profiles/r04/reference_cpu_timing.json)."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK")}
    env.update(OLPE_BENCH_SAMPLER="bench_stub:StubSampler", OLPE_STUB_MS="5",
               PYTHONPATH=os.pathsep.join([TESTS, REPO]))
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--config", "0",
                        "--full", "--no-alt"], cwd=REPO, env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    d = _line(r)
    c = d["config"]
    assert c["walkers_per_gpu"] == 1 and c["image"] == "32x32" and c["iters_per_step"] == 1000
    assert c["chain_stride"] == 1 and d["steps"] == 1
    assert d["posterior"]["walkers"] == 1 and d["posterior"]["gr_rc_max"] is None
    cb = d["cpu_baseline"]
    assert cb["cores"] == 1 and cb["kind"] == "port" and "1000 iterations" in cb["sample"]
    if os.path.exists("/opt/conda/bin/python3.9"):
        # the reference's loop cost measured here: the astropy-object oracle on one core,
        # beside the port under the same interpreter (one reference figure,
        # its ratio like for like); the build container's ratio stays a record only
        rl = cb["reference_like"]
        assert rl["cores"] == 1 and "1000 iterations" in rl["sample"] and rl["value"] > 0
        assert d["gpu_over_reference_like"] == pytest.approx(d["value"] / rl["value"])
        p39 = rl["port_same_interpreter"]
        assert p39["cores"] == 1 and "--port" in p39["sample"]
        assert rl["reference_over_port_same_interpreter"] == pytest.approx(
            rl["value"] / p39["value"])
        assert 0 < rl["reference_over_port_same_interpreter"] < 1
        assert "gpu_over_reference" not in d and "reference_value_derived" not in cb
        assert 0 < cb["build_container_reference_timing"]["reference_over_port"] < 1
    else:
        assert 0 < cb["reference_over_port"] < 1
        assert cb["reference_value_derived"] == pytest.approx(
            cb["value"] * cb["reference_over_port"])
        assert d["gpu_over_reference"] == pytest.approx(d["value"] / cb["reference_value_derived"])


def test_per_config_defaults_cover_the_survey_runs():
    import bench
    # configs[0] 1,000 iterations, [1] 10,000 at stride 1, [2] 2,000 at
    # stride 10, [4] 500 at stride 10
    tot = {k: v["iters"] * v["steps"] for k, v in bench.DEFAULTS.items()}
    assert tot == {0: 1000, 1: 10000, 2: 2000, 3: 2000, 4: 500}
    assert [bench.DEFAULTS[k]["stride"] for k in (0, 1, 2, 4)] == [1, 1, 10, 10]


def test_share_gpu_ranks_sum_moments_over_the_host_group():
    r = _run(["--gpus", "3", "--share-gpu"])
    assert r.returncode == 0, r.stderr
    d = _line(r)
    assert d["n_gpus"] == 3 and d["config"]["devices"] == [0, 0, 0]
    assert d["allgather_ms"] is None                       # no RCCL on a shared GPU
    p = d["posterior"]
    assert p["walkers"] == 3 * WPG and p["rows_per_walker"] == (STEPS + 1) * ITERS // STRIDE
    assert p["means"]["xcs"] == pytest.approx(1.0)


def test_eight_ranks_name_configs3():
    """--gpus 8 at configs[2]'s 65,536 walkers per GPU is SURVEY 8(d)'s configs[3]."""
    r = _run(["--gpus", "8", "--walkers", "65536", "--steps", "1"], {"OLPE_STUB_MS": "2"})
    assert r.returncode == 0, r.stderr
    d = _line(r)
    assert d["config"]["workload"].startswith("configs[3]: 524,288 walkers")
    assert d["posterior"]["walkers"] == 524288
    assert d["comm"]["rccl_nranks"] == 8 and d["comm"]["rccl_ranks"] == list(range(8))
    assert d["comm"]["walkers_allreduced"] == 524288


def test_ranks_on_one_gpu_are_refused_without_share_gpu():
    # every process sees one GPU: each rank takes device 0 (per-rank visibility), and the
    # PCI ids show that the ranks share it -> exit 4 on every rank, no line
    r = _run(["--gpus", "2"], {"OLPE_STUB_NDEV": "1"})
    assert r.returncode == 4
    assert "ranks share a GPU" in r.stderr
    assert not [ln for ln in r.stdout.splitlines() if ln.startswith("{")]


def test_rank_device_choice():
    from olpefit_amd import dist
    assert [dist.rank_device(r, 8) for r in range(8)] == list(range(8))
    assert dist.rank_device(3, 1) == 0              # one visible GPU per process
    with pytest.raises(ValueError):
        dist.rank_device(5, 4)


def test_killed_launcher_takes_its_ranks_along():
    """SIGTERM to the launcher terminates its ranks (and a rank whose launcher dies gets
    SIGTERM from the kernel: PR_SET_PDEATHSIG), so no rank outlives it holding a GPU."""
    import signal
    import time
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    env.update(OLPE_BENCH_SAMPLER="bench_stub:StubSampler", OLPE_STUB_MS="500",
               PYTHONPATH=os.pathsep.join([TESTS, REPO]))
    p = subprocess.Popen([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "3",
                          "--walkers", "8", "--steps", "100", "--warmup", "0",
                          "--no-cpu-baseline", "--no-alt"], cwd=REPO, env=env,
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    time.sleep(4)
    kids = subprocess.run(["pgrep", "-P", str(p.pid)], capture_output=True, text=True)
    pids = [int(x) for x in kids.stdout.split()]
    assert len(pids) == 3
    p.send_signal(signal.SIGTERM)
    p.wait(timeout=30)
    assert p.returncode != 0
    deadline = time.time() + 20
    while time.time() < deadline and any(os.path.exists(f"/proc/{q}") and
                                         open(f"/proc/{q}/stat").read().split()[2] != "Z"
                                         for q in pids):
        time.sleep(0.2)
    assert not any(os.path.exists(f"/proc/{q}") and open(f"/proc/{q}/stat").read().split()[2] != "Z"
                   for q in pids)


def test_driver_launch_form_under_torchrun():
    """The driver's scaling command, `python -m torch.distributed.run --nnodes=1
    --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...`:
    the ranks come from torchrun's environment (the bench starts none itself) and rank 0
    prints the whole job's line."""
    import socket
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT",
                        "TORCHELASTIC_RUN_ID", "OLPE_BENCH_LAUNCHED")}
    env.update(OLPE_BENCH_SAMPLER="bench_stub:StubSampler", OLPE_STUB_MS="5",
               PYTHONPATH=os.pathsep.join([TESTS, REPO]))
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
                        "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", str(port), "bench.py", "--gpus", "2",
                        "--walkers", str(WPG), "--steps", "3", "--warmup", "1",
                        "--no-cpu-baseline", "--no-alt"],
                       cwd=REPO, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    d = _line(r)
    assert d["n_gpus"] == 2 and d["config"]["launcher"] == "environment"
    assert d["config"]["local_ranks"] == [0, 1] and d["allgather_ms"] is not None


def test_config3_names_its_part():
    r = _run(["--config", "3", "--gpus", "2", "--walkers", "65536", "--steps", "1"],
             {"OLPE_STUB_MS": "1"})
    assert r.returncode == 0, r.stderr
    w = _line(r)["config"]["workload"]
    assert w.startswith("configs[3]'s per-GPU shards on 2 GPUs") and "--gpus 8" in w


def test_csv_emission_reported_outside_the_timed_region():
    """CSV emission is timed separately -- the last launch's rows of up to
    4,096 walkers written as the reference's chain files (stub rows here); a --full
    figure."""
    r = _run(["--full"])
    assert r.returncode == 0, r.stderr
    c = _line(r)["csv_emission"]
    assert c["files"] == WPG and c["rows_per_file"] == ITERS // STRIDE + 1
    assert c["bytes"] > 0 and c["ms"] > 0 and c["mb_per_s"] > 0


def _run_plain(args):
    """bench.py with the stub sampler and none of the --no-... switches."""
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT",
                        "TORCHELASTIC_RUN_ID", "OLPE_BENCH_LAUNCHED")}
    env.update(OLPE_BENCH_SAMPLER="bench_stub:StubSampler", OLPE_STUB_MS="5",
               PYTHONPATH=os.pathsep.join([TESTS, REPO]))
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1",
                        "--walkers", str(WPG)] + args, cwd=REPO, env=env,
                       capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stderr
    return _line(r)


def test_plain_run_times_its_steps_and_nothing_else():
    """`bench.py --gpus 1 --steps N --warmup W`: the N timed steps and their line; the
    other eval mode, the CPU baselines, the CSV emission and the clock are --full's."""
    d = _run_plain(["--steps", "4", "--warmup", "2"])
    assert d["full"] is False and d["steps"] == 4 and d["warmup"] == 2
    for k in ("alt_eval", "cpu_baseline", "gpu_over_cpu", "csv_emission", "dump_outputs"):
        assert k not in d
    assert d["per_rank_clock_ghz"] == [None] and "clock_ghz_live" not in d["roofline"]
    assert d["metric"] == __import__("bench").METRIC and d["unit"] == "walker-steps/s"
    assert d["higher_is_better"] is True and d["dtype"] == "f64"
    # --steps sets the timed launches: 4 stub launches of 5 ms, the warm-up outside them
    assert 5.0 <= d["ms_per_step"] < 50.0
    assert d["value"] == pytest.approx(WPG * ITERS * 4 / (d["ms_per_step"] * 4e-3), rel=1e-9)
    assert d["posterior"]["rows_per_walker"] == (4 + 2) * ITERS // STRIDE


def test_full_run_adds_the_other_measurements():
    """(the CPU baselines under --full: test_config0_line_beside_one_core)"""
    d = _run_plain(["--steps", "2", "--warmup", "1", "--full", "--no-cpu-baseline"])
    assert d["full"] is True and d["steps"] == 2
    assert d["alt_eval"]["eval"] == "exact" and d["alt_eval"]["value"] > 0
    assert d["csv_emission"]["files"] == WPG and d["per_rank_clock_ghz"] == [2.05]


def test_dump_outputs_writes_the_last_steps_arrays(tmp_path):
    """--dump-outputs DIR: float64 .npy files of the last timed step's chain rows, the
    walkers' state and counters and the moment sums, identical from run to run."""
    import numpy as np
    dirs = [str(tmp_path / "a"), str(tmp_path / "b")]
    lines = [_run_plain(["--steps", "2", "--warmup", "1", "--dump-outputs", d]) for d in dirs]
    info = lines[0]["dump_outputs"]
    nrec, ps = ITERS // STRIDE, 17
    assert info["walkers"] == info["of_walkers"] == WPG
    assert info["arrays"] == {"walkers": [WPG], "chain": [WPG, nrec, ps], "state": [WPG, ps],
                              "tries": [WPG, 16], "accepts": [WPG, 16], "moments": [85]}
    assert sorted(os.listdir(dirs[0])) == sorted(f"{k}.npy" for k in info["arrays"])
    total = 0
    for name, shape in info["arrays"].items():
        a, b = (np.load(os.path.join(d, name + ".npy")) for d in dirs)
        assert a.dtype == np.float64 and list(a.shape) == shape
        np.testing.assert_array_equal(a, b)
        total += os.path.getsize(os.path.join(dirs[0], name + ".npy"))
    assert total <= 64 * 10 ** 6
    # the stub's walkers carry their seed in column 0 of every row
    chain = np.load(os.path.join(dirs[0], "chain.npy"))
    np.testing.assert_array_equal(chain[:, -1, 0], 1000 + np.arange(WPG))
    np.testing.assert_array_equal(np.load(os.path.join(dirs[0], "state.npy")), chain[:, -1])


def test_dump_outputs_samples_a_large_ensemble_the_same_way_every_time(tmp_path, monkeypatch):
    """An output above the dump's byte budget is sampled by walker: the same seeded
    sample in every run, the same walkers in every per-walker array."""
    import numpy as np
    import bench
    sys.path.insert(0, TESTS)
    try:
        from bench_stub import StubSampler
    finally:
        sys.path.remove(TESTS)
    s = StubSampler(np.zeros((64, 64)))
    s.seed(1000 + np.arange(500))
    s.set_state(np.arange(17.0))
    s.ms = 0.0
    s.run_async(100, record_stride=10)
    s.moments_accumulate()
    per_walker = 8 * (1 + 10 * 17 + 17 + 2 * 16)
    monkeypatch.setattr(bench, "DUMP_BUDGET", 120 * per_walker + 85 * 8 + 7)   # + the moments
    a = bench.dump_outputs(s, str(tmp_path / "a"))
    b = bench.dump_outputs(s, str(tmp_path / "b"))
    assert a["walkers"] == b["walkers"] == 120 and a["of_walkers"] == 500
    assert a["bytes"] <= bench.DUMP_BUDGET
    wa, wb = (np.load(str(tmp_path / d / "walkers.npy")) for d in "ab")
    np.testing.assert_array_equal(wa, wb)
    assert len(set(wa)) == 120 and np.all(np.diff(wa) > 0) and 0 <= wa[0] and wa[-1] < 500
    np.testing.assert_array_equal(np.load(str(tmp_path / "a" / "state.npy"))[:, 0], 1000 + wa)
    np.testing.assert_array_equal(np.load(str(tmp_path / "a" / "chain.npy"))[:, 3, 0], 1000 + wa)


def test_per_rank_kernel_times_and_host_overhead_at_world8():
    """Verdict r04 item 5: a scaling shortfall is attributable from the line.  Rank r's
    stub launches take 20 + 2r ms, so per_rank_kernel_ms spans 20..34 and
    host_overhead_frac = 1 - max kernel ms x steps / the max-over-ranks timed region."""
    r = _run(["--gpus", "8", "--full"], {"OLPE_STUB_MS_PER_RANK": "2"})     # --full: the clock
    assert r.returncode == 0, r.stderr
    d = _line(r)
    k = d["per_rank_kernel_ms"]
    assert k["ranks"] == pytest.approx([20.0 + 2 * i for i in range(8)])
    assert k["min"] == pytest.approx(20.0) and k["max"] == pytest.approx(34.0)
    elapsed = d["ms_per_step"] * STEPS * 1e-3
    assert d["host_overhead_frac"] == pytest.approx(1 - 34e-3 * STEPS / elapsed, rel=1e-9)
    assert 0 <= d["host_overhead_frac"] < 0.5
    e = d["per_rank_elapsed_s"]
    assert e["max"] == pytest.approx(elapsed, rel=1e-9) and 0 < e["min"] <= e["max"]
    # the slowest rank sets the step: at least its 34 ms per launch
    assert d["ms_per_step"] >= 34.0
    # every rank's SMU clock over its timed launches; one warm-up launch of 20 ms is too
    # soon after the run's start for the telemetry, so the roofline leaves it out
    assert d["per_rank_clock_ghz"] == pytest.approx([2.05] * 8)
    assert d["clock_settled"] is False and "clock_ghz_live" not in d["roofline"]


def test_one_rank_line_carries_the_attribution_fields():
    # 0.4 s of 20 ms warm-up launches: settled (--full: the clock is sampled)
    r = _run(["--warmup", "20", "--full"])
    assert r.returncode == 0, r.stderr
    d = _line(r)
    assert d["per_rank_kernel_ms"]["ranks"] == pytest.approx([20.0])
    assert 0 <= d["host_overhead_frac"] < 1
    assert d["clock_settled"] is True and d["per_rank_clock_ghz"] == pytest.approx([2.05])
    f = d["roofline"]
    assert f["clock_ghz_live"] == pytest.approx(2.05)
    if "frac" in f:
        assert f["frac_of_held_clock_live"] == pytest.approx(f["frac"] * 2.4 / 2.05)


def test_identical_nodes_repeating_bus_ids_are_not_a_shared_gpu():
    """two nodes report the same PCI bus id for their GPU 0 -- one rank per
    node is one process per GPU (accepted); two ranks on one node's GPU are refused."""
    r = _run(["--gpus", "2"], {"OLPE_STUB_NDEV": "1", "OLPE_STUB_NODES": "2"})
    assert r.returncode == 0, r.stderr
    d = _line(r)
    assert d["config"]["devices"] == [0, 0] and len(d["config"]["pci_bus_ids"]) == 1
    assert d["config"]["nodes"] == 2
    r = _run(["--gpus", "3"], {"OLPE_STUB_NDEV": "1", "OLPE_STUB_NODES": "2"})
    assert r.returncode == 4 and "ranks share a GPU" in r.stderr


@pytest.mark.parametrize("args,world,start", [
    (["--walkers", "2048", "--gpus", "2"], 2, "custom: 2 x 2,048 walkers"),
    (["--walkers", "65536", "--gpus", "2"], 2, "configs[2]'s shape per GPU, weak-scaled over 2"),
    (["--walkers", "524288", "--steps", "1"], 1, "custom: 1 x 524,288 walkers"),
    (["--walkers", "65536", "--gpus", "8", "--steps", "1"], 8, "configs[3]: 524,288 walkers"),
    # verdict r05 item 3: configs[4] is 131,072 walkers on 8 GPUs -- one GPU runs a shard
    (["--config", "4", "--walkers", "16384", "--steps", "1"], 1,
     "configs[4]'s per-GPU shard on 1 GPU (16,384 of 131,072 walkers"),
    (["--config", "4", "--walkers", "16384", "--gpus", "2", "--steps", "1"], 2,
     "configs[4]'s shape per GPU, weak-scaled over 2 GPUs"),
    (["--config", "4", "--walkers", "16384", "--gpus", "8", "--steps", "1"], 8,
     "configs[4]: 131,072 walkers sharded 8 x MI355X"),
])
def test_workload_names_what_ran(args, world, start):
    """Verdict r04 item 2: the workload names a BASELINE config only at its shape."""
    r = _run(args, {"OLPE_STUB_MS": "1"})
    assert r.returncode == 0, r.stderr
    d = _line(r)
    assert d["n_gpus"] == world and d["config"]["workload"].startswith(start)
