"""replay/node_fleet: R robots on ONE host thread, the R alignments of a step in one launch (NDTFrame::alignBatch ->
ndtpso_map_align_batch).  alignBatch promises to be observably identical to the align() calls it stands for, so the pose logs of
a fleet are byte for byte those of the same program calling align() R times (NODE_FLEET_SEQUENTIAL=1), and a fleet of one robot
is node_replay."""
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import FRAME_M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "host")
N_SCANS, SEED = 12, 7


@pytest.fixture(scope="module")
def scans(tmp_path_factory):
    from ndtpso_slam_amd import synth
    rng = np.random.default_rng(4)
    s = np.linspace(0.0, 0.9, N_SCANS)
    poses = np.stack([2.0 + 1.2 * s, -1.0 + 0.8 * np.sin(1.5 * s), 0.3 + 0.25 * s], axis=1)
    clean = synth.raycast(poses)
    ranges = np.where(clean > 0, clean + rng.normal(0, 0.01, clean.shape), 0.0).astype(np.float32)
    path = tmp_path_factory.mktemp("fleet") / "scans.bin"
    with open(path, "wb") as f:
        np.array([N_SCANS, synth.N_BEAMS], dtype=np.int32).tofile(f)
        np.array([synth.ANGLE_MIN, synth.ANGLE_INC, synth.RANGE_MAX], dtype=np.float32).tofile(f)
        ranges.tofile(f)
    return path


def _fleet(scans, robots, prefix, env):
    r = subprocess.run([os.path.join(HOST, "replay", "node_fleet"), str(scans), str(FRAME_M), "0.5", "50", "30", str(SEED),
                        str(robots), str(prefix)], text=True, capture_output=True, env=env, timeout=300)
    assert r.returncode == 0 and '"failed_alignments": 0' in r.stdout, (r.stdout, r.stderr[-2000:])
    return [open("%s.%d.poses" % (prefix, k), "rb").read() for k in range(robots)]


@pytest.mark.parametrize("score", ["f64", None])          # the fp64 score; the default exact mode
def test_fleet_equals_the_sequential_calls_and_one_robot_equals_node_replay(scans, tmp_path, score):
    env = {k: v for k, v in os.environ.items() if k not in ("NDTPSO_SCORE", "NODE_FLEET_SEQUENTIAL")}
    if score:
        env["NDTPSO_SCORE"] = score
    batch = _fleet(scans, 5, tmp_path / "batch", env)
    seq = _fleet(scans, 5, tmp_path / "seq", dict(env, NODE_FLEET_SEQUENTIAL="1"))
    assert batch == seq
    assert len({b for b in batch}) == 5 and all(len(b.splitlines()) == N_SCANS for b in batch)      # five different robots
    one = _fleet(scans, 1, tmp_path / "one", env)
    replay = subprocess.check_output([os.path.join(HOST, "replay", "node_replay"), str(scans), str(FRAME_M), "0.5", "50", "30",
                                      str(SEED)], env=env)
    assert one[0] == replay


def _run(scans, robots, prefix, env, cell):
    r = subprocess.run([os.path.join(HOST, "replay", "node_fleet"), str(scans), str(FRAME_M), cell, "50", "30", str(SEED),
                        str(robots), str(prefix)], text=True, capture_output=True, env=env, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[-2000:])
    logs = [open("%s.%d.poses" % (prefix, k), "rb").read() for k in range(robots)]
    return logs, json.loads(r.stdout.strip().splitlines()[-1]), r.stderr


@pytest.mark.parametrize("how", ["a job fails", "no device map"])
def test_failures_inside_a_launch_are_the_sequential_calls_failures(scans, tmp_path, how):
    """alignBatch's own failure handling, with scans loaded on the device so that the requests really share a launch.  "a job
    fails": maps whose point pool is 64 chunks and cannot grow run out (as in tests/test_gpu_resident.py), and from then on the
    alignments against them come back from the launch with NDTPSO_E_CAPACITY as their jobs' rc (30 of the 33 alignments when
    this was written: the count is the sequential calls', whatever it is).  "no device map": a pool larger than
    the library accepts (refused before anything is allocated), so no reference frame gets its map and every request fails alone.  Either way: the guess is returned, the update that follows is refused, the process lives,
    and logs and counts are those of align() called R times."""
    env = {k: v for k, v in os.environ.items() if k not in ("NDTPSO_SCORE", "NODE_FLEET_SEQUENTIAL", "NDTPSO_ABORT_ON_ERROR")}
    env["NDTPSO_MAP_POOL_FIXED"] = "1"
    env["NDTPSO_MAP_POOL_MB"] = "0.03125" if how == "a job fails" else str(64 << 20)       # 64 chunks of 512 bytes; 64 TB
    batch, db, eb = _run(scans, 3, tmp_path / "batch", env, "0.5")
    seq, ds, es = _run(scans, 3, tmp_path / "seq", dict(env, NODE_FLEET_SEQUENTIAL="1"), "0.5")
    assert batch == seq
    assert db["failed_alignments"] == ds["failed_alignments"] > 0, (db, ds)
    if how == "no device map":
        assert db["failed_alignments"] == 3 * (N_SCANS - 1), db          # no alignment can run
    for err in (eb, es):
        assert "align failed" in err and "update after a failed align" in err, err[-1500:]
