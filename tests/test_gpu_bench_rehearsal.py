"""`python bench.py --gpus N` end to end with N > 1 rank processes on the ONE GPU of the test box: self-launch, process group,
row sharding of the chunk-wise synthetic data, the statistics all-reduce inside mlhip_em_iterate / mlhip_kmeans_step, the
max-over-ranks timing and the single JSON line. The transport is gloo on the host (`--allreduce gloo`): RCCL refuses two ranks
on one device, so the NCCL call itself is the only piece this cannot exercise (tests/test_gpu_rccl.py runs it with one rank).
The sharded job must reproduce the single-process numbers."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*args):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


def test_two_rank_em_line_matches_the_single_rank_run():
    # --full: at 400 000 rows an iteration is too short for events inside the timed region, the kernel times need the replay
    one = _bench("--samples", "400000", "--steps", "3", "--warmup", "1", "--no-cpu-baseline", "--full")
    two = _bench("--gpus", "2", "--allreduce", "gloo", "--n", "400000", "--steps", "3", "--warmup", "1", "--full")
    # two ranks on the ONE GPU of this box: `n_gpus` counts physical GPUs, `units` the ranks; the line says it is a rehearsal
    assert two["n_gpus"] == 1 and two["units"] == 2 and "rehearsal" in two
    assert two["n_local"] == [200000, 200000] and two["steps"] == 3
    a, b = one["config"]["final_mean_log_likelihood"], two["config"]["final_mean_log_likelihood"]
    assert abs(a - b) <= 1e-12 * abs(a)
    assert "roofline" in two and two["roofline"]["kernel_ms"]["em_estep"] > 0
    # the fields a first multi-GPU run is diagnosed with: every line has them, a single rank reports no all-reduce time
    for line in (one, two):
        assert line["ms_per_step_min"] <= line["ms_per_step_max"] <= line["ms_per_step"] * 1.5 + 1.0
        assert len(line["allreduce_ms_per_rank"]) == line["units"]
    assert one["allreduce_ms"] == 0
    assert one["roofline"]["exp_runs_in"].startswith("em_mstats")        # d = 32, K = 64: self-normalising statistics kernel


def test_three_rank_kmeans_and_diag_lines():
    one = _bench("--workload", "kmeans", "--samples", "600000", "--steps", "3", "--warmup", "1", "--no-cpu-baseline")
    three = _bench("--gpus", "3", "--allreduce", "gloo", "--workload", "kmeans", "--samples", "600000", "--steps", "3", "--warmup", "1")
    assert three["n_local"] == [200000, 200000, 200000]
    assert abs(one["config"]["inertia"] - three["config"]["inertia"]) <= 1e-12 * one["config"]["inertia"]
    d1 = _bench("--workload", "em-diag", "--samples", "300000", "--steps", "3", "--warmup", "1", "--no-cpu-baseline")
    d3 = _bench("--gpus", "3", "--allreduce", "gloo", "--workload", "em-diag", "--samples", "300000", "--steps", "3", "--warmup", "1")
    a, b = d1["config"]["final_mean_log_likelihood"], d3["config"]["final_mean_log_likelihood"]
    assert abs(a - b) <= 1e-12 * abs(a)


@pytest.mark.parametrize("workload,n", [("em", 400000), ("em-diag", 300000)])
def test_dumped_outputs_are_the_last_timed_step(tmp_path, workload, n):
    """--dump-outputs writes what the primary workload's last timed step returned: warmup + steps iterations of mlhip_em_iterate
    from the benchmark's start, and the same bytes on a second run with the same arguments (em-diag: the kernel times come from a
    replay of the steps after the timed region in a --full run, which must not leak into the dump)."""
    import numpy as np
    from ml_amd import _lib, synth
    sys.path.insert(0, ROOT)
    import bench
    diagonal = workload == "em-diag"
    runs = []
    for r in range(2):
        out = tmp_path / f"run{r}"
        line = _bench("--workload", workload, "--samples", str(n), "--steps", "3", "--warmup", "1", "--no-cpu-baseline",
                      "--full", "--dump-outputs", str(out))
        assert line["steps"] == 3 and line["ms_per_step"] > 0
        runs.append({f[:-4]: np.load(out / f) for f in sorted(os.listdir(out))})
    cov_name = "variances" if diagonal else "covariances"
    assert sorted(runs[0]) == sorted(["log_likelihood", "mixing", "means", cov_name])
    assert all(a.dtype == np.float64 for a in runs[0].values())
    for name in runs[0]:
        assert np.array_equal(runs[0][name], runs[1][name]), name

    d, K = (16, 16) if diagonal else (32, 64)
    mix = synth.Mixture(d, K, diagonal=diagonal)
    ctx = _lib.Context(0)
    data = _lib.Data(ctx, bench.sample_rows(mix, 0, n))
    _, cov = data.sample_covariance()
    S0 = np.stack([np.diag(cov)] * K) if diagonal else np.stack([cov] * K)
    steps, _, ll, pi, mu, S, _ = data.em_iterate(np.full(K, 1.0 / K), mix.initial_means(), S0, 4, 0.0, 0.0, diagonal)
    data.close()
    ctx.close()
    got = runs[0]
    assert steps == 4 and abs(got["log_likelihood"][0] - ll) <= 1e-12 * abs(ll)
    for name, want in (("mixing", pi), ("means", mu), (cov_name, S)):
        assert np.max(np.abs(got[name] - want)) <= 1e-11 * np.max(np.abs(want)), name


def test_a_plain_run_measures_the_headline_alone():
    """Without --full the line is the headline's: no CPU baseline, and no kernel times where they would take a replay of their
    own (400 000 rows: too short an iteration for events inside the timed region). --full adds them; the timed steps and what
    they compute are the same either way."""
    args = ("--samples", "400000", "--steps", "3", "--warmup", "1")
    plain = _bench(*args)
    full = _bench(*args, "--full", "--cpu-samples", "2000")
    for key in ("cpu_baseline", "cpu_baseline_all_cores", "secondary", "roofline", "allreduce_ms"):
        assert key not in plain, key
    assert full["cpu_baseline"]["value"] > 0 and full["roofline"]["kernel_ms"]["em_estep"] > 0 and full["allreduce_ms"] == 0
    for key in ("metric", "unit", "higher_is_better", "dtype", "steps", "warmup", "n_gpus"):
        assert plain[key] == full[key], key
    assert plain["value"] > 0 and plain["ms_per_step"] > 0
    assert plain["config"]["final_mean_log_likelihood"] == full["config"]["final_mean_log_likelihood"]
