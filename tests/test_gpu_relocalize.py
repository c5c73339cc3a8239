"""NDTFrame::relocalize through host/replay/relocalize_check on the verified case of tests/search_case.py: a pose lattice is
searched on the device, its best eight nodes are refined in one launch, and the frame tracks on from the result.

The oracle's side of it is the same procedure spelt out with the reference's own functions: cost_function at every node, the
best eight, pso_optimization from each with deviation step / 2 and consecutive slices of the srand(11) stream, the lowest cost,
and one more pso_optimization from there with align()'s first-call deviation and the next slice."""
import os
import subprocess

import numpy as np
import pytest

import search_case as sc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "host", "replay", "relocalize_check")
SEED = 11
FIRST_CALL = (0.1, 0.1, 3.1415e-3)
ENV_OFF = ("NDTPSO_SCORE", "NDTPSO_RESIDENT", "NDTPSO_ALIGN_FRAME_CONFIG")


@pytest.fixture(scope="module")
def scans(tmp_path_factory):
    from ndtpso_slam_amd import synth
    maps, query = sc.ranges()
    path = tmp_path_factory.mktemp("relocalize") / "scans.bin"
    with open(path, "wb") as f:
        np.array([len(maps) + 1, sc.N_BEAMS], dtype=np.int32).tofile(f)
        np.array([synth.ANGLE_MIN, sc.angle_inc(), synth.RANGE_MAX], dtype=np.float32).tofile(f)
        maps.tofile(f)
        query.tofile(f)
    return path


def _run(scans, env):
    args = [EXE, str(scans), str(sc.FRAME_M), str(sc.FRAME_M), repr(sc.CELL_SIDE), str(SEED), str(sc.TOP_K), str(len(sc.MAP_POSES))]
    args += [repr(float(v)) for v in sc.ORIGIN + sc.STEP] + [str(v) for v in sc.COUNT]
    args += [repr(float(v)) for pose in sc.MAP_POSES for v in pose]
    r = subprocess.run(args, text=True, capture_output=True, env=env, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[-2000:])
    return r


def _parse(stdout):
    out = {}
    for line in stdout.splitlines():
        w = line.split()
        if w[0] == "relocalize":
            out.update(ok=int(w[2]), hits=int(w[4]), pose=np.array([float.fromhex(v) for v in w[6:9]]), cost=float.fromhex(w[10]),
                       pose_hex=w[6:9], cost_hex=w[10])
        elif w[0] == "align":
            out.update(next=np.array([float.fromhex(v) for v in w[1:4]]), next_hex=w[1:4])
        elif w[0] == "errors":
            out.update(errors=int(w[1]), refused=int(w[3]), last=" ".join(w[5:]))
    return out


@pytest.fixture(scope="module")
def oracle_side(oracle):
    ref, new, costs = sc.oracle_case()
    from ndtpso_slam_amd import capi
    poses = capi.lattice_poses(sc.ORIGIN, sc.STEP, sc.COUNT)
    best = np.argsort(costs, kind="stable")[:sc.TOP_K]
    cfg = oracle.PSOConfig.make()
    n_draw = 3 + 3 * 30 + 6 * 30 * 50
    stream = oracle.glibc_rand(SEED, (sc.TOP_K + 1) * n_draw)
    refined = [ref.pso(poses[i], new, tuple(s / 2 for s in sc.STEP), cfg, table=stream[k * n_draw:(k + 1) * n_draw])
               for k, i in enumerate(best)]
    won = min(range(sc.TOP_K), key=lambda k: (refined[k][1], k))
    pose, cost = refined[won][0], refined[won][1]
    nxt = ref.pso(pose, new, FIRST_CALL, cfg, table=stream[sc.TOP_K * n_draw:])[0]
    plain = ref.pso((2.5, -1.6, 0.75), new, FIRST_CALL, cfg, seed=SEED)[0]
    return pose, cost, nxt, plain


def test_oracle_relocalizes_where_plain_pso_does_not(oracle_side):
    pose, cost, nxt, plain = oracle_side
    truth = np.array(sc.TRUTH)
    assert np.hypot(*(pose[:2] - truth[:2])) < 0.02 and abs(pose[2] - truth[2]) < 0.005, pose
    assert np.hypot(*(plain[:2] - truth[:2])) > 0.5, plain


def test_relocalize_equals_the_oracle_in_both_score_modes(scans, oracle_side):
    pose, cost, nxt, _ = oracle_side
    base = {k: v for k, v in os.environ.items() if k not in ENV_OFF}
    got = {}
    for score in ("exact", "f64"):
        g = got[score] = _parse(_run(scans, dict(base, NDTPSO_SCORE=score)).stdout)
        assert g["ok"] == 1 and g["hits"] == sc.TOP_K, g
        assert np.abs(g["pose"] - pose).max() <= 1e-9, (score, g["pose"], pose)
        assert abs(g["cost"] - cost) <= 1e-9 * abs(cost), (score, g["cost"], cost)
        assert np.abs(g["next"] - nxt).max() <= 1e-9, (score, g["next"], nxt)
    for key in ("pose_hex", "cost_hex", "next_hex"):
        assert got["exact"][key] == got["f64"][key], (key, got)


def test_a_frame_that_is_not_resident_fails_loudly(scans):
    env = {k: v for k, v in os.environ.items() if k not in ENV_OFF + ("NDTPSO_ABORT_ON_ERROR",)}
    r = _run(scans, dict(env, NDTPSO_RESIDENT="0"))
    g = _parse(r.stdout)
    assert g["ok"] == 0 and g["hits"] == 0 and g["cost"] == 0.0, g
    assert g["pose"].tolist() == list(sc.ORIGIN), g
    assert g["errors"] == 1 and g["refused"] == 1, g
    assert "update after a failed align" in g["last"], g
    assert "relocalize: the frame is not resident" in r.stderr, r.stderr[-2000:]
