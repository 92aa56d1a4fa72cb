"""bench.py's --dump-outputs files (what the timed path computed, 64 MB at most, a fixed sample of anything larger), its workload
cache (one file per version of the generator sources) and what a plain run leaves to --full, on the CPU; on the GPU, that the files
hold the last timed step's values and that --full adds its records without changing them."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
import beast_mcmc_amd as bm
from beast_mcmc_amd.inputs import patterns

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_writes_float64_arrays_by_name(tmp_path):
    site = np.linspace(-3.0, -1.0, 1000)
    written = bench.dump_outputs(str(tmp_path / "out"), {"lnL": [-1234.5], "site_lnL": site})
    assert written == {"lnL": 1, "site_lnL": 1000}
    lnl = np.load(tmp_path / "out" / "lnL.npy")
    assert lnl.dtype == np.float64 and lnl.tolist() == [-1234.5]
    back = np.load(tmp_path / "out" / "site_lnL.npy")
    assert back.dtype == np.float64 and np.array_equal(back, site)


def test_dump_of_a_large_output_is_a_fixed_sample_within_the_limit(tmp_path):
    big = np.arange(bench.DUMP_LIMIT_BYTES // 8 + 12345, dtype=np.float64)       # more than the whole limit on its own
    a = bench.dump_outputs(str(tmp_path / "a"), {"lnL": [1.0], "site_lnL": big})
    b = bench.dump_outputs(str(tmp_path / "b"), {"lnL": [1.0], "site_lnL": big})
    assert a == b and a["site_lnL"] < big.size
    total = sum(os.path.getsize(os.path.join(tmp_path / "a", f)) for f in os.listdir(tmp_path / "a"))
    assert total <= bench.DUMP_LIMIT_BYTES
    sa, sb = np.load(tmp_path / "a" / "site_lnL.npy"), np.load(tmp_path / "b" / "site_lnL.npy")
    assert np.array_equal(sa, sb)                                   # the same entries every run
    assert np.all(np.diff(sa) > 0) and np.all(np.isin(sa, big))      # in increasing order, taken from the output itself


def test_workload_cache_file_follows_the_generator_sources(tmp_path):
    d = str(tmp_path / "cache")
    f = bench.workload_cache_file(d, "A", 1.0, "coalescent")
    assert os.path.isdir(d) and os.path.dirname(f) == d
    assert f == bench.workload_cache_file(d, "A", 1.0, "coalescent")
    assert f != bench.workload_cache_file(d, "B", 1.0, "coalescent")
    assert bench.workload_cache_file("", "A", 1.0, "coalescent") is None


def test_a_plain_run_is_the_default_and_keeps_no_workload_file():
    plain = bench.parse_args(["--gpus", "1", "--steps", "5", "--warmup", "2"])
    assert plain.full is False and plain.cache is None
    assert bench.parse_args(["--full"]).full is True


def test_other_configs_are_full_child_runs_sharing_the_cache(monkeypatch):
    """--full's other configurations: each a child `bench.py --full` (its own CPU baseline and traffic passes) reading and writing
    the parent run's workload directory."""
    import types
    cmds = []

    def fake_run(cmd, **kw):
        cmds.append(cmd)
        line = {"value": 1.0, "unit": "evals/s", "steps": int(cmd[cmd.index("--steps") + 1]), "roofline": {}, "cpu_baseline": {"value": 0.5}}
        return types.SimpleNamespace(returncode=0, stdout="banner\n" + json.dumps(line) + "\n", stderr="")
    monkeypatch.setattr(subprocess, "run", fake_run)
    args = bench.parse_args(["--full"])
    args.cache = "/nonexistent/workloads"
    rec = bench.other_configs(args)
    assert [c[c.index("--config") + 1] for c in cmds] == ["B", "C", "D", "E"]
    for c in cmds:
        assert "--full" in c and c[c.index("--cache") + 1] == "/nonexistent/workloads"
    assert all(rec[k]["value"] == 1.0 and rec[k]["cpu_baseline"] == {"value": 0.5} for k in "BCDE")


def test_steps_below_one_is_refused():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--steps" in r.stderr


class _Ranks:
    """Stands in for torch.distributed in gather_ranks: every rank's object, as all_gather_object would hand them over."""

    def __init__(self, objects):
        self.objects = objects

    def get_world_size(self):
        return len(self.objects)

    def all_gather_object(self, out, mine):
        out[:] = self.objects


@pytest.mark.parametrize("world", [1, 2, 3])
def test_gathered_site_values_are_in_pattern_order_whatever_the_rank_count(world):
    counts = [5, 3, 8]                                              # patterns per partition (config E: partition after partition)
    whole = np.arange(sum(counts), dtype=np.float64)
    starts = np.concatenate([[0], np.cumsum(counts)[:-1]])
    rows = []
    for r in range(world):                                          # rank r: block r of every partition (PartitionedWorkload.shard)
        blocks = [whole[s0 + a:s0 + b] for s0, n in zip(starts, counts) for a, b in [patterns.shard_bounds(n, world)[r]]]
        rows.append((np.concatenate(blocks), [len(b) for b in blocks]))
    assert np.array_equal(bench.gather_ranks(_Ranks(rows), rows[0][0], rows[0][1]), whole)
    plain = [(whole[a:b], [b - a]) for a, b in patterns.shard_bounds(len(whole), world)]      # configs A-D: one block per rank
    assert np.array_equal(bench.gather_ranks(_Ranks(plain), plain[0][0]), whole)


class _Unwritable:
    def __reduce__(self):
        raise OSError("no space left on device")


def test_cache_that_cannot_be_written_costs_only_the_cache(tmp_path):
    cache = str(tmp_path / "wl.pkl")
    made = []

    def maker():
        made.append(1)
        return {"x": _Unwritable()}
    wl = bench.load_workload(cache, maker)
    assert made == [1] and isinstance(wl["x"], _Unwritable)
    assert os.listdir(tmp_path) == []                                # no cache file, no partial file
    assert bench.load_workload(cache, lambda: [1.5]) == [1.5]         # written ...
    assert bench.load_workload(cache, lambda: [2.5]) == [1.5]         # ... and read back
    open(cache, "wb").write(b"not a pickle")
    assert bench.load_workload(cache, lambda: [3.5]) == [3.5]         # an unreadable file: generated again


SHORT = ["--no-cpu-baseline", "--no-live-traffic", "--no-library-route", "--no-side-records", "--no-other-configs"]


def _bench(out_dir, *args, env=None, switches=SHORT):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--warmup", "2", "--dump-outputs", str(out_dir)]
                       + switches + list(args), capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    return line, {f[:-4]: np.load(os.path.join(out_dir, f)) for f in os.listdir(out_dir)}


@pytest.mark.gpu
def test_dump_holds_the_last_timed_step(tmp_path):
    """config D on the benchmark1 alignment: the models cycle with the step number, so 3 and 4 timed steps end on different
    models; each dump is its own line's lnL, and its site values sum (pattern weights) to that lnL."""
    weights = bm.synth.from_pattern_fixture(os.path.join(ROOT, "tests", "golden", "benchmark1_patterns.npz")).weights
    seen = []
    for steps in (3, 4):
        line, d = _bench(tmp_path / str(steps), "--config", "D", "--real", "benchmark1", "--steps", str(steps))
        assert line["steps"] == steps and line["ms_per_step"] > 0
        assert set(d) == {"lnL", "site_lnL"} and d["lnL"].dtype == np.float64 and d["site_lnL"].shape == weights.shape
        assert d["lnL"].tolist() == [line["lnL"]]
        assert abs(float(np.dot(weights, d["site_lnL"])) - line["lnL"]) <= 1e-11 * abs(line["lnL"])
        seen.append(line["lnL"])
    assert seen[0] != seen[1]


@pytest.mark.gpu
def test_partitioned_dump_and_its_sharded_code_path(tmp_path):
    """config E: the per-partition values sum to lnL, each partition's site values sum (weights) to its value; the multi-GPU code
    path (process group, all-reduce, gathered site values) dumps the same numbers."""
    pw = bm.synth.config_e()
    line, d = _bench(tmp_path / "plain", "--config", "E", "--steps", "3", "--cache", str(tmp_path / "cache"))
    assert set(d) == {"lnL", "partition_lnL", "site_lnL"} and d["partition_lnL"].shape == (len(pw.parts),)
    assert d["lnL"].tolist() == [line["lnL"]]
    assert abs(float(d["partition_lnL"].sum()) - line["lnL"]) <= 1e-12 * abs(line["lnL"])
    for k, piece in enumerate(np.split(d["site_lnL"], np.cumsum(pw.pattern_counts)[:-1])):
        assert abs(float(np.dot(pw.parts[k].weights, piece)) - d["partition_lnL"][k]) <= 1e-11 * abs(d["partition_lnL"][k])
    import socket
    with socket.socket() as sk:                                     # a process group of one rank on a free port
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    _, ds = _bench(tmp_path / "sharded", "--config", "E", "--steps", "3", "--cache", str(tmp_path / "cache"), "--force-sharded", env=env)
    assert np.array_equal(d["partition_lnL"], ds["partition_lnL"]) and np.array_equal(d["site_lnL"], ds["site_lnL"])
    assert abs(float(ds["lnL"][0]) - line["lnL"]) <= 1e-12 * abs(line["lnL"])     # (the sum over partitions taken on the device)


@pytest.mark.gpu
def test_full_adds_its_records_and_leaves_the_headline_steps_alone(tmp_path):
    """config D on the benchmark1 alignment: a plain run carries none of --full's records and measures no traffic of its own; a
    --full run carries them, and its timed steps compute the same numbers, to the bit, as the plain run's."""
    real = ("--config", "D", "--real", "benchmark1", "--steps", "3")
    plain, dp = _bench(tmp_path / "plain", *real, switches=[])
    assert plain["full"] is False and plain["steps"] == 3 and plain["ms_per_step"] > 0
    assert plain["cpu_baseline"] is None and plain["other_caller"] is None and plain["partial_update"] is None
    assert "measured in this run" not in plain["roofline"]["traffic_source"]
    full, df = _bench(tmp_path / "full", *real, "--cpu-seconds", "1", switches=["--full", "--no-live-traffic"])
    assert full["full"] is True
    assert full["cpu_baseline"]["gpu_vs_cpu_site_lnL_max_rel_err"] <= 1e-10
    assert full["other_caller"]["caller"] == "btl" and "error" not in full["partial_update"]
    assert full["lnL"] == plain["lnL"] and full["lnL_first_eval"] == plain["lnL_first_eval"]
    assert set(df) == set(dp) and all(np.array_equal(df[k], dp[k]) for k in dp)
