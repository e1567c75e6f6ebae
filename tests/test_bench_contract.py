"""bench.py's contract with the driver, held without a GPU by RUNNING bench.py: ``--selftest-cpu`` takes the same code path — launcher, rank set-up, shard
construction, warm-up, timed region, all-gather, JSON line, and with ``--full`` the whole-schedule walk, batch-1 latency, PCIe-inclusive loop and CPU-baseline
workers — on the CPU port
(``oracle/cpu_port``, test infrastructure) with gloo and tiny sizes.  The numbers are meaningless and the line says so (``selftest``, ``metric``); what is
checked is the layout of the line, the arithmetic between its fields and that ``--gpus N`` launches N ranks.  Result-valued assertions (no instance lost over
the schedule, ...) live in the GPU tests (tests/test_gpu_bench_config.py)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
SMALL = ["--steps", "2", "--warmup", "1", "--batch", "2", "--horizon", "6", "--model", "reduced", "--cold-iters", "100", "--regions", "1",
         "--latency-ticks", "6", "--schedule-ticks", "8"]


@pytest.fixture(scope="module")
def cpu_lib():
    from tests import _cpu_port
    _cpu_port.load()  # (builds it on demand)
    return os.path.join(_cpu_port.PORT_DIR, "libmpc_cpu.so")


def _run(args, timeout=600):
    out = subprocess.run([sys.executable, BENCH] + args, capture_output=True, text=True, timeout=timeout, cwd=ROOT,
                         env={k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")})
    rows = [l for l in out.stdout.split("\n") if l.startswith("{")]
    return out, rows


def test_command_line_parses():
    out = subprocess.run([sys.executable, BENCH, "--help"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0
    for flag in ("--gpus", "--steps", "--warmup", "--no-floor", "--corrector-prim-tol", "--refine-appended-knot", "--walk-generator", "--no-whole-schedule"):
        assert flag in out.stdout, flag


def test_refuses_a_cpu_library_outside_the_selftest(cpu_lib):
    out, rows = _run(["--lib", cpu_lib] + SMALL)
    assert out.returncode != 0 and not rows and "HIP library only" in out.stderr


def test_line_of_the_cpu_rehearsal_has_the_contract_keys(cpu_lib):
    out, rows = _run(["--selftest-cpu", "--lib", cpu_lib, "--full"] + SMALL)
    assert out.returncode == 0, out.stderr[-2000:]
    assert len(rows) == 1, "bench.py prints ONE JSON line"
    d = json.loads(rows[0])
    assert d["selftest"] is True and "NOT a measurement" in d["metric"] and d["metric"].startswith("mpc_solves_per_sec")
    assert d["unit"] == "solves/s" and d["higher_is_better"] is True and d["scaling"] == "weak"
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1 and d["vs_baseline"] is None and d["dtype"] == "f64" and d["data"] == "synthetic"
    assert abs(d["value"] - 2 * 1e3 / d["ms_per_step"]) < 0.02 * d["value"]          # value = instances per tick / time per tick
    assert "workload" in d["config"] and "model" not in d["config"] and "parallelism" in d["config"]
    # the objects the judge reads come before the supplementary ones (the driver's record keeps a bounded number of key names)
    keys = list(d)
    for k in ("roofline", "cpu_baseline", "whole_schedule", "whole_schedule_plain_warm_start", "whole_schedule_exact_iteration_budget", "roofline_whole_tick",
              "value_with_result_download", "per_rank_ms_per_step", "ensemble_allgather"):
        assert k in d and keys.index(k) < 26, k
    assert d["roofline"] is None and d["roofline_whole_tick"] is None   # (the CPU port times no kernels: the rooflines are the GPU run's)
    c = d["cpu_baseline"]
    assert c["kind"] in ("port", "reference") and c["unit"] == "solves/s" and c["cores"] >= 1 and c["value"] > 0 and len(c["sample"]) > 20 and d["cpu_baseline_note"] is None
    w = d["whole_schedule"]
    assert w["ticks"] == 8 and set(w["ms_per_tick"]) >= {"mean", "p50", "p90", "p95", "max"} and "instance_losses" in w and "nominal_instance_lost" in w
    for k in ("whole_schedule_plain_warm_start", "whole_schedule_exact_iteration_budget"):
        assert d[k]["ticks"] == 8 and "instance_losses" in d[k]
    assert d["whole_schedule_exact_iteration_budget"]["settings"]["corrector_prim_tol"] == 0.0 and d["whole_schedule_exact_iteration_budget"]["settings"]["refine_appended_knot"] == 0
    v = d["value_with_result_download"]
    assert v["unit"] == "solves/s" and v["bytes_downloaded_per_step"] > 0 and abs(v["value"] - 2 * 1e3 / v["ms_per_step"]) < 0.02 * v["value"]
    assert d["per_rank_ms_per_step"] == {"min": d["ms_per_step"], "max": d["ms_per_step"], "ranks": 1}
    assert d["p50_ms_per_solve_batch1"] > 0 and d["latency_ticks"] == 6
    assert set(d["measurements"]) >= {"frozen_references", "walk"}


def test_plain_run_measures_the_headline_only(cpu_lib):
    """Without ``--full`` the line keeps its layout and its headline, and everything that takes runs of its own is null: no supplementary
    measurement, no latency, no whole schedule, no download loop, no CPU baseline."""
    out = subprocess.run([sys.executable, BENCH, "--help"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "--full" in out.stdout
    out, rows = _run(["--selftest-cpu", "--lib", cpu_lib] + SMALL)
    assert out.returncode == 0, out.stderr[-2000:]
    assert len(rows) == 1, "bench.py prints ONE JSON line"
    d = json.loads(rows[0])
    assert d["selftest"] is True and d["metric"].startswith("mpc_solves_per_sec") and d["unit"] == "solves/s" and d["higher_is_better"] is True
    assert d["steps"] == 2 and d["warmup"] == 1 and d["dtype"] == "f64"
    assert abs(d["value"] - 2 * 1e3 / d["ms_per_step"]) < 0.02 * d["value"]
    assert set(d["measurements"]) == {"frozen_references", "walk"}
    assert d["value"] == min(m["value"] for m in d["measurements"].values())      # the headline is the lower of the two
    for k in ("cpu_baseline", "whole_schedule", "whole_schedule_plain_warm_start", "whole_schedule_exact_iteration_budget", "value_with_result_download",
              "p50_ms_per_solve_batch1", "p90_ms_per_solve_batch1", "p95_ms_per_solve_batch1"):
        assert k in d and d[k] is None, k
    assert d["latency_ticks"] == 0 and "--full" in d["cpu_baseline_note"]
    assert d["per_rank_ms_per_step"] == {"min": d["ms_per_step"], "max": d["ms_per_step"], "ranks": 1}


def test_gpus_n_launches_n_ranks(cpu_lib):
    """``python bench.py --gpus 2`` without a launcher around it: the parent starts two ranks (gloo here, RCCL on the GPUs), relays rank 0's line."""
    out, rows = _run(["--selftest-cpu", "--lib", cpu_lib, "--gpus", "2", "--no-latency", "--no-whole-schedule"] + SMALL)
    assert out.returncode == 0, out.stderr[-2000:]
    assert len(rows) == 1
    d = json.loads(rows[0])
    assert d["n_gpus"] == 2 and d["selftest"] is True
    g = d["ensemble_allgather"]
    assert g["instances"] == 4 and g["complete"] is True and g["finite"] is True   # ids 0 .. 3: rank r holds r, r + 2
    p = d["per_rank_ms_per_step"]
    assert p["ranks"] == 2 and p["min"] <= p["max"] and abs(p["max"] - d["ms_per_step"]) < 1e-3   # ms_per_step = the slowest rank's
    assert abs(d["value"] - 2 * 2 * 1e3 / d["ms_per_step"]) < 0.02 * d["value"]    # whole-job rate: both ranks' instances
    assert d["cpu_baseline"] is None and "N = 1" in d["cpu_baseline_note"]
    assert "sharded over 2 GPU(s)" in d["config"]["parallelism"]


def test_launcher_fails_when_a_rank_fails(cpu_lib):
    out, rows = _run(["--selftest-cpu", "--lib", "/nonexistent/libmpc.so", "--gpus", "2", "--no-latency", "--no-whole-schedule", "--no-cpu-baseline"] + SMALL)
    assert out.returncode != 0 and not rows


def test_launcher_does_not_wait_for_a_rendezvous_that_cannot_happen(cpu_lib):
    """One rank dies before it joins (on the GPU box: `--gpus 2` where there is one GPU): the other would wait ten minutes for it at the rendezvous.  The launcher
    ends it at once and fails."""
    import time
    t0 = time.time()
    out = subprocess.run([sys.executable, BENCH, "--selftest-cpu", "--lib", cpu_lib, "--gpus", "2", "--no-latency", "--no-whole-schedule", "--no-cpu-baseline"] + SMALL,
                         capture_output=True, text=True, timeout=300, cwd=ROOT, env=dict({k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE")}, MPC_BENCH_TEST_FAIL_RANK="1"))
    assert out.returncode != 0 and time.time() - t0 < 120 and "ranks failed" in out.stderr


def test_steps_are_the_timed_steps_and_the_dump_repeats(cpu_lib, tmp_path):
    """Without --regions the region of --steps ticks is timed once; --dump-outputs writes the last timed tick of every measurement, the same
    numbers in two runs with the same arguments."""
    args = ["--selftest-cpu", "--lib", cpu_lib, "--no-latency", "--no-whole-schedule", "--no-cpu-baseline"] + SMALL[:SMALL.index("--regions")] + SMALL[SMALL.index("--regions") + 2:]
    dumps = []
    for run in ("a", "b"):
        out, rows = _run(args + ["--dump-outputs", str(tmp_path / run)])
        assert out.returncode == 0, out.stderr[-2000:]
        d = json.loads(rows[0])
        assert d["steps"] == 2 and d["timed_regions"] == 1
        dumps.append({f: np.load(str(tmp_path / run / f)) for f in sorted(os.listdir(str(tmp_path / run)))})
    a, b = dumps
    assert sorted(a) == sorted("%s_%s.npy" % (m, k) for m in d["measurements"] for k in ("xs", "us", "K0", "k0"))
    for f, x in a.items():
        assert x.dtype == np.float64 and x.shape[0] == 2 and np.isfinite(x).all(), f
        assert np.array_equal(x, b[f]), f
    assert a["walk_xs.npy"].shape == (2, 7, 57) and a["walk_us.npy"].shape == (2, 6, 22) and a["walk_K0.npy"].shape == (2, 22, 56)


def test_dump_above_the_limit_keeps_one_seeded_sample_of_instances(tmp_path):
    import bench
    B = 50
    outputs = {m: {"xs": np.arange(B * 300, dtype=float).reshape(B, 300) + i, "K0": np.arange(B * 100, dtype=float).reshape(B, 10, 10)} for i, m in enumerate(("frozen", "walk"))}
    rows = bench.dump_outputs(str(tmp_path / "a"), outputs, limit=60000)
    assert 1 <= len(rows) < B and np.all(np.diff(rows) > 0)
    assert sum(os.path.getsize(str(tmp_path / "a" / f)) for f in os.listdir(str(tmp_path / "a"))) <= 60000
    for m, o in outputs.items():
        for k, x in o.items():
            assert np.array_equal(np.load(str(tmp_path / "a" / ("%s_%s.npy" % (m, k)))), x[rows])
    assert np.array_equal(bench.dump_outputs(str(tmp_path / "b"), outputs, limit=60000), rows)
    assert len(bench.dump_outputs(str(tmp_path / "c"), outputs)) == B
