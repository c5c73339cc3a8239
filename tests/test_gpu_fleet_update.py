"""replay/node_fleet with every phase of a step batched (NDTFrame::loadLaserBatch, alignBatch, updateBatch), and
replay/update_batch_check.  The batch entries promise to be observably identical to the member calls they stand for, so the pose
logs of a fleet are byte for byte the same whichever phases are batched -- all of them (the default), all but the updates
(NODE_FLEET_UPDATE=calls), all but the loads (NODE_FLEET_LOAD=calls), none (NODE_FLEET_SEQUENTIAL=1) -- and a fleet of one robot
is node_replay.  The scans are the recipe of tests/test_gpu_fleet.py."""
import os
import subprocess

import numpy as np
import pytest

from conftest import FRAME_M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "host")
N_SCANS, SEED = 12, 7
FLEET_ENV = ("NDTPSO_SCORE", "NODE_FLEET_SEQUENTIAL", "NODE_FLEET_LOAD", "NODE_FLEET_UPDATE")


@pytest.fixture(scope="module")
def scans(tmp_path_factory):
    from ndtpso_slam_amd import synth
    rng = np.random.default_rng(4)
    s = np.linspace(0.0, 0.9, N_SCANS)
    poses = np.stack([2.0 + 1.2 * s, -1.0 + 0.8 * np.sin(1.5 * s), 0.3 + 0.25 * s], axis=1)
    clean = synth.raycast(poses)
    ranges = np.where(clean > 0, clean + rng.normal(0, 0.01, clean.shape), 0.0).astype(np.float32)
    path = tmp_path_factory.mktemp("fleet_update") / "scans.bin"
    with open(path, "wb") as f:
        np.array([N_SCANS, synth.N_BEAMS], dtype=np.int32).tofile(f)
        np.array([synth.ANGLE_MIN, synth.ANGLE_INC, synth.RANGE_MAX], dtype=np.float32).tofile(f)
        ranges.tofile(f)
    return path


def _fleet(scans, robots, cell, prefix, env):
    r = subprocess.run([os.path.join(HOST, "replay", "node_fleet"), str(scans), str(FRAME_M), cell, "50", "30", str(SEED),
                        str(robots), str(prefix)], text=True, capture_output=True, env=env, timeout=300)
    assert r.returncode == 0 and '"failed_alignments": 0' in r.stdout and '"device_errors": 0' in r.stdout, (r.stdout, r.stderr[-2000:])
    return [open("%s.%d.poses" % (prefix, k), "rb").read() for k in range(robots)], r.stdout


@pytest.mark.parametrize("cell", ["0.5", "0.25"])
@pytest.mark.parametrize("score", ["f64", None])          # the fp64 score; the default exact mode
def test_pose_logs_do_not_depend_on_which_phases_are_batched(scans, tmp_path, score, cell):
    env = {k: v for k, v in os.environ.items() if k not in FLEET_ENV}
    if score:
        env["NDTPSO_SCORE"] = score
    batch, out = _fleet(scans, 5, cell, tmp_path / "batch", env)
    assert '"load": "batch", "update": "batch"' in out, out
    assert len(set(batch)) == 5 and all(len(b.splitlines()) == N_SCANS for b in batch)      # five different robots
    for name, extra in (("update_calls", {"NODE_FLEET_UPDATE": "calls"}), ("load_calls", {"NODE_FLEET_LOAD": "calls"}),
                        ("sequential", {"NODE_FLEET_SEQUENTIAL": "1"})):
        other, out = _fleet(scans, 5, cell, tmp_path / name, dict(env, **extra))
        assert other == batch, name
    one, _ = _fleet(scans, 1, cell, tmp_path / "one", env)
    replay = subprocess.check_output([os.path.join(HOST, "replay", "node_replay"), str(scans), str(FRAME_M), cell, "50", "30",
                                      str(SEED)], env=env, timeout=300)
    assert one[0] == replay


def test_batch_entries_equal_the_member_calls_on_twin_frames(scans):
    """replay/update_batch_check: batchable requests, a frame that owns a map as the scan, a frame repeated in one call, a frame of
    another thread's context, requests after a failed align -- through loadLaserBatch / updateBatch and through the member calls."""
    env = {k: v for k, v in os.environ.items() if k not in FLEET_ENV + ("NDTPSO_ABORT_ON_ERROR", "NDTPSO_RESIDENT")}
    r = subprocess.run([os.path.join(HOST, "replay", "update_batch_check"), str(scans)], text=True, capture_output=True, env=env,
                       timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), (r.returncode, r.stdout[-3000:], r.stderr[-2000:])
    assert "refused 1" in r.stdout and "errors recorded 4" in r.stdout, r.stdout        # the failed align and three refused updates
    assert "update after a failed align" in r.stderr
