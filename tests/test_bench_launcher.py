"""bench.py's rank launcher and multi-rank plumbing, on CPU (gloo, world size 2): rank -> device map and
environment, the refusal of a --gpus / WORLD_SIZE mismatch, and -- through `--dry-run`, which runs everything
of the multi-rank path except the solver -- rendezvous, MAX-reduced region time, the final gather through
sharding.gather_results and `n_gpus` in the JSON line; both scaling modes and both workloads through the same
dry run; and the supervisor: a rank that dies before the rendezvous ends the job promptly instead of hanging it."""
import json
import os
import subprocess
import sys
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_launch_plan():
    assert bench.launch_plan(1, {}) == ("single", 0, 1)
    assert bench.launch_plan(4, {}) == ("spawn", 0, 4)
    assert bench.launch_plan(4, {"WORLD_SIZE": "4", "RANK": "3"}) == ("worker", 3, 4)
    assert bench.launch_plan(1, {"WORLD_SIZE": "1", "RANK": "0"}) == ("single", 0, 1)
    assert bench.launch_plan(8, {"WORLD_SIZE": "2", "RANK": "0"})[0] == "error"
    assert bench.launch_plan(0, {})[0] == "error"


def test_rank_env_maps_one_device_per_rank():
    for r in range(4):
        e = bench.rank_env(r, 4, 29511, base={"PATH": "/usr/bin"})
        assert e["RANK"] == str(r) and e["LOCAL_RANK"] == str(r) and e["WORLD_SIZE"] == "4"
        assert e["MASTER_ADDR"] == "127.0.0.1" and e["MASTER_PORT"] == "29511"
        assert e["HSA_ENABLE_IPC_MODE_LEGACY"] == "0" and e["PATH"] == "/usr/bin"


def _clean_env():
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    return env


def test_spawned_world2_dry_run_reports_two_ranks():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dry-run"], env=_clean_env(),
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1  # rank 0 alone prints
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["gather_ok"] is True and d["gathered_rows"] == 9
    assert abs(d["region_s_max"] - 0.002) < 1e-12  # MAX over ranks of (rank + 1) ms


def test_world_size_mismatch_is_refused():
    env = _clean_env()
    env.update(WORLD_SIZE="4", RANK="0")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dry-run"], env=env,
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 2 and "WORLD_SIZE" in out.stderr


def _dry(*flags, timeout=300):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--dry-run", *flags], env=_clean_env(),
                         capture_output=True, text=True, timeout=timeout)
    return out


def test_dry_run_strong_scaling_splits_one_global_batch():
    out = _dry("--gpus", "2", "--scaling", "strong", "--batch", "4097")
    assert out.returncode == 0, out.stderr[-2000:]
    d = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][0])
    assert d["scaling"] == "strong" and d["global_batch"] == 4097 and d["batch_rank0"] == 2049
    assert d["sum_of_rank_batches"] == 4097  # contiguous shards cover the global batch exactly once


def test_dry_run_weak_scaling_and_drone_defaults():
    out = _dry("--gpus", "2")
    d = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][0])
    assert d["scaling"] == "weak" and d["batch_rank0"] == 4096 and d["global_batch"] == 8192 and d["sum_of_rank_batches"] == 8192
    out = _dry("--gpus", "2", "--workload", "drone400")
    d = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][0])
    # BASELINE config 5: 8192 trajectories in all, strong scaling by default (1024 per GPU on 8)
    assert d["workload"] == "drone400" and d["scaling"] == "strong" and d["global_batch"] == 8192 and d["batch_rank0"] == 4096
    a = bench.parse_args(["--workload", "drone400"])
    assert (a.batch, a.horizon, a.scaling) == (8192, 400, "strong")
    a = bench.parse_args([])
    assert (a.batch, a.horizon, a.scaling, a.repeats, a.fresh_regions, a.mode) == (4096, 200, "weak", 2, 0, "ms")
    # BASELINE configs 2 and 4 at their stated sizes (secondary lines); the SO3 script runs the SS solver
    a = bench.parse_args(["--workload", "so3"])
    assert (a.batch, a.horizon, a.scaling, a.mode) == (1, 100, "weak", "ss")
    a = bench.parse_args(["--workload", "so3", "--mode", "ms", "--batch", "256"])
    assert (a.batch, a.mode) == (256, "ms")
    a = bench.parse_args(["--workload", "al1024"])
    assert (a.batch, a.horizon, a.scaling, a.mode) == (1024, 200, "weak", "ms")


def test_rank_dying_before_rendezvous_ends_the_job_promptly():
    """Rank 1 exits 3 before init_process_group: rank 0 would wait in the rendezvous; the supervisor must take it
    down and return the failure, well inside the rendezvous timeout."""
    t0 = time.monotonic()
    out = _dry("--gpus", "2", "--dry-run-fail-rank", "1", timeout=120)
    dt = time.monotonic() - t0
    assert out.returncode == 3, (out.returncode, out.stderr[-1000:])
    assert dt < 60, dt
    assert not [ln for ln in out.stdout.splitlines() if ln.startswith("{")]  # no result line from a failed job


def test_supervisor_deadline_kills_stuck_ranks():
    procs = [subprocess.Popen([sys.executable, "-c", "import time; time.sleep(300)"]) for _ in range(2)]
    t0 = time.monotonic()
    rc = bench.supervise(procs, deadline_s=1.0)
    assert rc == 124 and time.monotonic() - t0 < 30
    assert all(p.poll() is not None for p in procs)


def test_lib_override_is_refused_without_the_flag(tmp_path):
    env = _clean_env()
    env["TOLG_HIP_LIB"] = str(tmp_path / "other.so")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "1"], env=env, capture_output=True,
                         text=True, timeout=300)
    assert out.returncode != 0 and "--allow-lib-override" in (out.stderr + out.stdout)


def test_profile_lookups_pick_the_fast_sweep_and_fresh_series_shape():
    """bench.py's helpers that read the committed profiles: since round 4 the backward sweep is two kernels and the headline's
    dominant one is the fast sweep (`k_backward3<.., true>`); the executed-fp64 figure sums it and the fused launch; the fresh-solve
    series reports the median of the regions without per-kernel events."""
    ks = {"void tolg::k_backward3<6, false, false, false>": {"SQ_WAVES": 1024.0, "SQ_INSTS_VALU_FMA_F64": 1.0},
          "void tolg::k_backward3<6, false, false, true>": {"SQ_WAVES": 1024.0, "SQ_INSTS_VALU_FMA_F64": 2.0},
          "void tolg::k_rollout_lin<6>": {"SQ_WAVES": 1024.0, "SQ_INSTS_VALU_FMA_F64": 3.0}}
    name, v = bench._pick_kernel(ks, "k_backward3")
    assert name.endswith("true>") and v["SQ_INSTS_VALU_FMA_F64"] == 2.0
    assert bench._pick_kernel(ks, "k_rollout_lin")[0].endswith("k_rollout_lin<6>")
    assert bench._pick_kernel({"void tolg::k_backward3<6, false, false>": {}}, "k_backward3")[0].endswith("false>")   # round-3 profiles
    assert bench._pick_kernel(ks, "k_nothing") == (None, None)
    fr = bench.fresh_series([(0.012, True, (0.30, 0.25, 0.0)), (0.011, False, None), (0.013, True, (0.31, 0.24, 0.0)), (0.0115, False, None)],
                            20, 5, 1.0, 1, 0.54)
    assert fr["regions"] == 4 and fr["median_ms_per_step"] == pytest.approx(0.5625) and fr["value"] == pytest.approx(20 / 0.01125)
    assert fr["kernel_ms_per_step"]["backward"] == pytest.approx(0.305) and fr["ratio_to_headline_ms_per_step"] == pytest.approx(0.5625 / 0.54)
    ex = bench.executed_fp64_fraction(0.54)   # from the committed profiles/*_sq_mix.json
    assert ex is None or (0.1 < ex["frac"] < 1.0 and len(ex["kernels"]) == 2)


def test_steps_are_the_timed_steps_in_all():
    """--steps K times exactly K steps: the regions of --repeats split them, sizes within one of each other."""
    assert bench.region_sizes(20, 2) == [10, 10]
    assert bench.region_sizes(7, 3) == [3, 2, 2]
    assert bench.region_sizes(3, 200) == [1, 1, 1]
    assert bench.region_sizes(1, 2) == [1]
    for K in range(1, 40):
        for R in (1, 2, 3, 5, 200):
            s = bench.region_sizes(K, R)
            assert sum(s) == K and max(s) - min(s) <= 1 and len(s) == min(K, R)
    for bad in (["--steps", "0"], ["--repeats", "0"]):
        with pytest.raises(SystemExit):
            bench.parse_args(bad)


def test_dump_sample_is_fixed_and_within_budget():
    np = pytest.importorskip("numpy")
    assert list(bench.dump_sample(10, 100)) == list(range(10))
    row = 8 * (201 * 22 + 200 * 6 + 4)   # SE3, N = 200: xs_q, xs_xi, us, J, iters, status, index
    a, b = bench.dump_sample(4096, row), bench.dump_sample(4096, row)
    assert np.array_equal(a, b) and len(a) * row <= bench.DUMP_BYTES_MAX < (len(a) + 1) * row
    assert len(np.unique(a)) == len(a) and np.all(np.diff(a) > 0) and a[-1] < 4096


def test_dump_outputs_writes_the_caller_arrays_in_float64(tmp_path):
    """The writer on a result shaped like the solver's (host tensors): names, dtypes, the last iteration's cost."""
    import types
    import numpy as np
    import torch
    B, N, m, K = 5, 4, 6, 3
    g = torch.Generator().manual_seed(0)
    res = types.SimpleNamespace(xs_q=torch.rand(B, N + 1, 4, 4, generator=g, dtype=torch.float64),
                                xs_xi=torch.rand(B, N + 1, 6, generator=g, dtype=torch.float64),
                                us=torch.rand(B, N, m, generator=g, dtype=torch.float64),
                                J_hist=torch.arange(B * K, dtype=torch.float64).reshape(B, K),
                                iters=torch.tensor([3, 3, 1, 2, 3], dtype=torch.int32), status=torch.zeros(B, dtype=torch.int32))
    info = bench.dump_outputs(res, str(tmp_path / "d"))
    got = {f[:-4]: np.load(os.path.join(info["dir"], f)) for f in info["files"]}
    assert set(got) == {"xs_q", "xs_xi", "us", "J", "iters", "status", "trajectory_index"}
    assert all(a.dtype == np.float64 for a in got.values()) and info["trajectories"] == B and info["sample"] == "all"
    assert np.array_equal(got["xs_q"], res.xs_q.numpy()) and np.array_equal(got["us"], res.us.numpy())
    assert list(got["J"]) == [2.0, 5.0, 6.0, 10.0, 14.0] and list(got["iters"]) == [3, 3, 1, 2, 3]
    assert info["bytes"] == sum(os.path.getsize(os.path.join(info["dir"], f)) for f in info["files"]) <= bench.DUMP_BYTES_MAX


@pytest.mark.gpu
def test_dump_outputs_are_the_same_whatever_the_region_split(tmp_path):
    """Two runs with the same arguments but a different split of the timed steps compute the same outputs, bit for bit, and
    the line counts exactly --steps timed steps; 2048 x 200 is larger than the 64 MB dump, so the seeded sample is taken."""
    import numpy as np
    lines, dumps = [], []
    for rep in ("1", "3"):
        d = str(tmp_path / ("r" + rep))
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "7", "--warmup", "2", "--repeats", rep,
                              "--batch", "2048", "--no-cpu-baseline", "--dump-outputs", d], env=_clean_env(), capture_output=True,
                             text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        lines.append(json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][0]))
        dumps.append({f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))})
    for ln, rep in zip(lines, (1, 3)):
        tr = ln["config"]["timed_regions"]
        assert ln["steps"] == 7 and tr["steps_in_all"] == 7 and tr["repeats"] == rep and ln["ms_per_step"] > 0
        assert ln["config"]["dump_outputs"]["bytes"] <= bench.DUMP_BYTES_MAX
    a, b = dumps
    assert set(a) == set(b) == {"xs_q", "xs_xi", "us", "J", "iters", "status", "trajectory_index"}
    assert 0 < len(a["trajectory_index"]) < 2048 and np.all(a["iters"] == 9) and np.all(a["status"] == 0)
    assert sum(os.path.getsize(os.path.join(str(tmp_path / "r1"), f)) for f in os.listdir(str(tmp_path / "r1"))) <= bench.DUMP_BYTES_MAX
    for k in a:
        assert a[k].dtype == np.float64 and np.array_equal(a[k], b[k]), k
