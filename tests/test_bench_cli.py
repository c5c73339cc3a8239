"""bench.py's command line: a plain run carries the headline and nothing that takes runs of its own (those are behind
--full), and --dump-outputs writes what the last timed step computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_writes_float64_arrays_of_the_results(tmp_path):
    """bench._dump_outputs: pose, cost and, out of the AlignStats words, status (flags only: the arbitration count of its
    upper half is not a result) and n_points -- float64 .npy files, nothing else."""
    import bench
    from ndtpso_slam_amd import capi
    B = 5
    st = np.zeros(B, dtype=capi.STATS_DTYPE)
    st["n_points"] = np.arange(B) + 1000
    st["status"] = [0, 0, 2, 0, 1]
    st["arbitrated"] = 7
    st["t_start"], st["t_end"] = 123456, 234567
    pose, cost = np.arange(3.0 * B).reshape(B, 3) / 7, np.arange(float(B)) / 3
    raw = st.view(np.int32).reshape(B, 8)          # as the benchmark holds them: the device's int32 words
    d = tmp_path / "out" / "nested"
    bench._dump_outputs(str(d), capi, pose, cost, raw)
    assert sorted(os.listdir(d)) == ["cost.npy", "n_points.npy", "pose.npy", "status.npy"]
    got = {n: np.load(d / (n + ".npy")) for n in ("pose", "cost", "status", "n_points")}
    assert all(a.dtype == np.float64 for a in got.values())
    assert np.array_equal(got["pose"], pose) and np.array_equal(got["cost"], cost)
    assert got["status"].tolist() == [0, 0, 2, 0, 1] and got["n_points"].tolist() == [1000, 1001, 1002, 1003, 1004]


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_last_steps_outputs(tmp_path, ctx):
    """One small plain run (16 pairs, 20 x 10 PSO, 3 timed steps): the contract's fields, none of --full's measurements, and
    in --dump-outputs' directory the poses and costs of the very pairs the arguments stand for -- bit for bit what
    ndtpso_align_pairs returns for them."""
    from ndtpso_slam_amd import capi, synth
    B, P, I = 16, 20, 10
    out = tmp_path / "dump"
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "NDTPSO_BENCH_FORCE_DIST")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--settle-ms", "0",
                        "--pairs", str(B), "--particles", str(P), "--iterations", str(I), "--dump-outputs", str(out)],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["unit"] == "alignments/s" and d["higher_is_better"] is True and d["steps"] == 3 and d["warmup"] == 1
    assert d["ms_per_step"] > 0 and abs(d["value"] - B * 1e3 / d["ms_per_step"]) <= 1e-9 * d["value"]
    assert d["untimed_launches_total"] == 1                                 # the one warm-up step: nothing else was launched first
    assert d["cpu_baseline"] is None and d["value_one_batch_at_a_time"] is None and d["roofline"]["kernel_ms"] is None
    assert d["extra"]["without_clock_settle"] is None
    assert not {"modes", "config5", "live_sequence", "single_pair_latency_ms"} & set(d["extra"])
    assert 0 < d["roofline"]["frac"] < 1 and d["extra"]["status_nonzero"] == 0

    p = synth.make_pairs(B, seed=2024, first_pair=0, total_pairs=B)
    geom = capi.ScanGeom(p.n_beams, float(p.angle_min), float(p.angle_inc), float(p.range_max), 0.1)
    pose, cost, st = ctx.align_pairs(p.ref_ranges, p.new_ranges, geom, capi.Grid(60, 60, 0.5), (0, 0, 0), (0.1, 0.1, 3.1415e-3),
                                     capi.PSOConfig.make(I, P), seeds=p.seeds, mode=capi.SCORE_EXACT)
    got = {n: np.load(out / (n + ".npy")) for n in ("pose", "cost", "status", "n_points")}
    assert all(a.dtype == np.float64 for a in got.values())
    assert got["pose"].shape == (B, 3) and np.array_equal(got["pose"], pose) and np.array_equal(got["cost"], cost)
    assert not got["status"].any() and np.array_equal(got["n_points"], st["n_points"].astype(np.float64))
