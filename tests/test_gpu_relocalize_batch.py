"""NDTFrame::relocalizeBatch through host/replay/relocalize_fleet_check: three robots with maps of their own are relocalized in ONE
call (one ndtpso_map_search_batch, one ndtpso_map_align_batch) and by relocalize() robot after robot; the two outputs must be
the same bytes.  Robot 0 is the verified case of tests/search_case.py with seed 11, first in the batch: its lines must be
relocalize_check's for the same arguments hex for hex, and that tool is held to the oracle (tests/test_gpu_relocalize.py)."""
import os
import subprocess

import numpy as np
import pytest

import search_case as sc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLEET = os.path.join(ROOT, "host", "replay", "relocalize_fleet_check")
SINGLE = os.path.join(ROOT, "host", "replay", "relocalize_check")
SEED = 11
ENV_OFF = ("NDTPSO_SCORE", "NDTPSO_RESIDENT", "NDTPSO_ALIGN_FRAME_CONFIG")
# robots 1 and 2: other query poses (scans 7 and 8 of the file), maps of their own at 0.5 m and 0.3 m cells
QUERIES = [(-2.5, 1.0, -0.3), (4.0, -1.5, 0.8)]


def _floats(values):
    return [repr(float(v)) for v in values]


def _robot(cell_side, resident, top_k, query, origin, step, count, map_scans):
    words = [str(sc.FRAME_M), str(sc.FRAME_M), repr(cell_side), str(int(resident)), str(top_k), str(query)]
    words += _floats(origin + step) + [str(v) for v in count] + [str(len(map_scans))]
    for m in map_scans:
        words += [str(m)] + _floats(sc.MAP_POSES[m])
    return words


def _fleet():
    return [_robot(sc.CELL_SIDE, True, sc.TOP_K, 6, sc.ORIGIN, sc.STEP, sc.COUNT, range(6)),
            _robot(0.5, True, 4, 7, (-3.1, 0.4, -0.5), (0.3, 0.3, 0.1), (5, 5, 5), range(6)),
            _robot(0.3, True, 5, 8, (3.4, -2.1, 0.6), (0.3, 0.3, 0.1), (5, 5, 5), range(4))]


def _fleet_with_failures():
    """six robots: runs of two and of three around a frame that is not resident (robot 2), and inside the second run a request
    whose lattice the search refuses (robot 4: an axis without nodes)"""
    good = _fleet()
    return [good[0], good[1],
            _robot(0.5, False, 4, 7, (-3.1, 0.4, -0.5), (0.3, 0.3, 0.1), (5, 5, 5), range(6)),
            good[2],
            _robot(0.5, True, 4, 7, (-3.1, 0.4, -0.5), (0.3, 0.3, 0.1), (0, 5, 5), range(6)),
            _robot(0.5, True, 3, 7, (-2.8, 0.7, -0.4), (0.3, 0.3, 0.1), (3, 3, 3), range(6))]


@pytest.fixture(scope="module")
def scans(tmp_path_factory):
    from ndtpso_slam_amd import synth
    maps, query = sc.ranges()
    more = np.stack([sc.scan(100 + k, pose) for k, pose in enumerate(QUERIES)])
    path = tmp_path_factory.mktemp("relocalize_fleet") / "scans.bin"
    with open(path, "wb") as f:
        np.array([len(maps) + 1 + len(more), sc.N_BEAMS], dtype=np.int32).tofile(f)
        np.array([synth.ANGLE_MIN, sc.angle_inc(), synth.RANGE_MAX], dtype=np.float32).tofile(f)
        maps.tofile(f)
        query.tofile(f)
        more.tofile(f)
    return path


def _run(args, env):
    r = subprocess.run(args, text=True, capture_output=True, env=env, timeout=300)
    assert r.returncode == 0, (args[0], r.returncode, r.stdout, r.stderr[-2000:])
    return r


def _run_fleet(path, scans, env, robots=None):
    robots = _fleet() if robots is None else robots
    return _run([FLEET, path, str(scans), str(SEED), str(len(robots))] + [w for r in robots for w in r], env)


def _by_robot(stdout):
    """{robot: its lines}, and the last line (behind the line of the stream's position, which only the comparison of the two
    outputs reads)"""
    lines = stdout.splitlines()
    assert lines[-2].startswith("rand "), lines[-2:]
    out, at = {}, None
    for line in lines[:-2]:
        if line.startswith("robot "):
            at = int(line.split()[1])
            out[at] = []
        else:
            out[at].append(line)
    return out, lines[-1]


@pytest.mark.parametrize("score", ["exact", "f64"])
def test_batch_is_the_member_calls_and_robot_0_is_the_single_tool(scans, score):
    env = dict({k: v for k, v in os.environ.items() if k not in ENV_OFF}, NDTPSO_SCORE=score)
    batch = _run_fleet("batch", scans, env)
    member = _run_fleet("member", scans, env)
    assert batch.stdout == member.stdout, (batch.stdout, member.stdout)
    robots, last = _by_robot(batch.stdout)
    assert sorted(robots) == [0, 1, 2]
    for r, lines in robots.items():
        assert len(lines) == 2 and lines[0].startswith("relocalize ok 1 hits %d " % (sc.TOP_K, 4, 5)[r]) and lines[1].startswith("align "), (r, lines)
    assert last.split()[:4] == ["errors", "0", "refused", "0"], last
    # robot 0 against relocalize_check with the same arguments
    args = [SINGLE, str(scans), str(sc.FRAME_M), str(sc.FRAME_M), repr(sc.CELL_SIDE), str(SEED), str(sc.TOP_K), "6"]
    args += _floats(sc.ORIGIN + sc.STEP) + [str(v) for v in sc.COUNT] + _floats([v for pose in sc.MAP_POSES for v in pose])
    single = _run(args, env)
    assert single.stdout.splitlines() == robots[0], (single.stdout, robots[0])


def test_requests_that_cannot_be_served_inside_and_between_runs(scans):
    """Robot 2's frame is not resident: its request takes the member call between two shared runs.  Robot 4's lattice has an axis
    without nodes: its search is refused inside a shared run.  Both fail as the member calls fail -- nothing drawn, the same error
    recorded with the same text, the next update() refused -- and the others keep the lines, and the rand() stream the position,
    that they have when the member calls are made in the same order."""
    env = {k: v for k, v in os.environ.items() if k not in ENV_OFF + ("NDTPSO_ABORT_ON_ERROR",)}
    env = dict(env, NDTPSO_SCORE="exact")
    batch = _run_fleet("batch", scans, env, _fleet_with_failures())
    member = _run_fleet("member", scans, env, _fleet_with_failures())
    assert batch.stdout == member.stdout, (batch.stdout, member.stdout)
    robots, last = _by_robot(batch.stdout)
    assert sorted(robots) == list(range(6))
    for r in (2, 4):
        assert robots[r][0].startswith("relocalize ok 0 hits 0 "), robots[r]
        w = robots[r][1].split()
        assert w[0] == "errors" and w[2] == "refused" and int(w[3]) == 1, robots[r]
        assert "update after a failed align" in robots[r][1], robots[r]
    assert "relocalize: the frame is not resident" in batch.stderr, batch.stderr[-2000:]
    for r, hits in ((0, sc.TOP_K), (1, 4), (3, 5), (5, 3)):
        assert robots[r][0].startswith("relocalize ok 1 hits %d " % hits) and robots[r][1].startswith("align "), robots[r]
    assert last.split()[:4] == ["errors", "2", "refused", "2"], last
    assert "a lattice axis without nodes" in last, last
    # robots 0 and 1 relocalize ahead of every failure: their lines are the all-good fleet's
    good, _ = _by_robot(_run_fleet("batch", scans, env).stdout)
    assert robots[0] == good[0] and robots[1] == good[1]
