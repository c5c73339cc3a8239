"""ndtpso_map_curvature / ndtpso_map_curvature_batch on the device: cost, gradient and Hessian of the score at a pose against the
restatement of the contract (tests/curvature_ref.py), the cost byte for byte ResidentMap.cost's in the fp64 score, on every
table plan, at every trip boundary, alone and in batches, and through the drop-in (NDTFrame::curvature / curvatureBatch).
Maps come from tests/search_case.py: 361 beams, 60 m / 0.5 m, six scans.

Tolerance everywhere (curvature_ref.tolerance): |got - want| <= 2^-53 (n_points + 64) M, M the sum of the absolute products."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import curvature_ref as cr
import search_case as sc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "host")


@pytest.fixture(scope="module")
def case(ctx):
    return sc.device_case(ctx)


def _poses():
    from ndtpso_slam_amd import capi
    lattice = capi.lattice_poses(sc.ORIGIN, sc.STEP, sc.COUNT)
    nodes = lattice[np.linspace(0, len(lattice) - 1, 16).astype(int)]
    return np.concatenate([[sc.TRUTH], nodes, [[1.3, -0.7, 7.0]], [[500.0, 0.0, 0.3]]])


def _ten(cv, i):
    return np.concatenate([[cv["cost"][i]], cv["gradient"][i], cv["hessian"][i]])


def _sum_bytes(cv):
    """the ten sums of every record, as bytes"""
    return b"".join(_ten(cv, i).tobytes() for i in range(len(cv["cost"])))


def _check_parity(ctx, m, s, poses, what=""):
    """cost == ResidentMap.cost(F64) byte for byte, n_hit the restatement's, the nine derivatives within the tolerance -- with the
    device's own sincos and exp in the restatement"""
    from ndtpso_slam_amd import capi
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
    cv = m.curvature(s, poses)
    costs = m.cost(s, poses, mode=capi.SCORE_F64)
    assert cv["cost"].tobytes() == costs.tobytes(), (what, cv["cost"], costs)
    xy = s.get()
    n = xy.shape[0]
    assert (cv["n_points"] == n).all()
    cells = cr.cells_of(m.cells())
    grid = (m.grid.width, m.grid.height, m.grid.cell_side)
    sn, cn = ctx.device_math("sincos", poses[:, 2])
    for i, pose in enumerate(poses):
        t = cr.point_terms(cells, grid, xy, pose, cn[i], sn[i])
        e = ctx.device_math("exp", t["x"]) if n else np.zeros(0)
        want, M, n_hit = cr.sums(t, e)
        got = _ten(cv, i)
        tol = cr.tolerance(n, M)
        print(what, "pose", pose, "n_hit", cv["n_hit"][i], n_hit, "max err / tol", np.max(np.abs(got - want) / np.maximum(tol, 1e-300)))
        assert cv["n_hit"][i] == n_hit, (what, pose)
        if np.isnan(want).any():
            assert np.isnan(got).all() and np.isnan(want).all(), (what, pose, got, want)
            continue
        assert (np.abs(got - want) <= tol).all(), (what, pose, got, want, tol)
    return cv


def test_parity(ctx, case):
    m, s = case
    poses = _poses()
    cv = _check_parity(ctx, m, s, poses, "parity")
    assert cv["n_hit"][0] > sc.N_BEAMS // 4                      # the truth: a pose with overlap
    assert cv["n_hit"][-1] == 0 and not _ten(cv, len(poses) - 1).any()      # 500 m away: nothing lands, all ten sums are zero
    assert (cv["path"] == 1).all()                               # 0.5 m cells: the bitmap in LDS, power-of-two form


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257])
def test_trip_boundaries(ctx, case, n):
    """the chunk, group-of-four and padding edges of the trips: prefixes of the query scan's points"""
    from ndtpso_slam_amd import capi
    m, s = case
    xy = s.get()
    p = capi.ResidentScan(ctx, max(n, 1))
    p.set(xy[:n])
    cv = _check_parity(ctx, m, p, _poses()[[0, 3, 17, 18]], "n = %d" % n)
    assert (cv["n_points"] == n).all()
    if n == 0:
        assert not _sum_bytes(cv).strip(b"\x00\x80") and (cv["n_hit"] == 0).all()       # all zeros (the cost: -0., as the cost call's)


@pytest.mark.parametrize("cell_side,pow2", [(0.25, True), (0.3, False)])
def test_every_table_plan(ctx, cell_side, pow2):
    """tests/test_gpu_map_search.py::test_every_table_plan's recipe: plans 1 / 0 with the bitmap in LDS, 5 / 4 from the HBM image"""
    from ndtpso_slam_amd import capi
    grid = capi.Grid(300, 300, cell_side)
    m = capi.ResidentMap(ctx, grid)
    s = capi.ResidentScan(ctx, sc.N_BEAMS)
    maps, query = sc.ranges()
    s.load_scan(maps[2], sc.geom(), clip=grid)
    m.insert(s, (0, 0, 0))
    s.load_scan(query, sc.geom(), clip=grid)
    inside = 0.05 + np.array([[0.01, 0.02], [0.05, 0.07], [0.1, 0.03], [0.12, 0.11]])
    poses = capi.lattice_poses((1.0, -1.0, 0.4), (0.2, 0.2, 0.05), (5, 3, 2))[::3]
    for reach, path in ((50.0, 1 if pow2 else 0), (140.0, 5 if pow2 else 4)):
        lo, hi = int((150.0 - reach) / cell_side), int((150.0 + reach) / cell_side)
        m.insert_host(np.concatenate([lo * cell_side - 150.0 + inside, hi * cell_side - 150.0 + inside]), (0, 0, 0))
        m.build()
        cv = _check_parity(ctx, m, s, poses, "cells %g reach %g" % (cell_side, reach))
        assert (cv["path"] == path).all(), (cv["path"], path)


def test_pure_function_of_map_scan_and_pose(ctx, case):
    """one pose alone, then at indices 0, 15, 16 and 999 among 1000 poses -- more poses than waves in flight can hold at once on
    the grid the launcher picks for them, so the stride loop runs: the 96 bytes are the same"""
    m, s = case
    pose = np.array(sc.TRUTH) + (0.01, -0.02, 0.003)
    alone = m.curvature(s, pose)["raw"].tobytes()
    assert len(alone) == 96
    rng = np.random.default_rng(3)
    many = np.array(sc.TRUTH) + rng.uniform(-1, 1, (1000, 3)) * (0.5, 0.5, 0.1)
    for at in (0, 15, 16, 999):
        many[at] = pose
    raw = m.curvature(s, many)["raw"]
    for at in (0, 15, 16, 999):
        assert raw[at].tobytes() == alone, at
    for n_poses in (1, 16, 17):
        part = m.curvature(s, many[:n_poses])["raw"]
        assert part.tobytes() == raw[:n_poses].tobytes(), n_poses


def test_batch(ctx):
    """jobs over three maps with a map and a scan each repeated, one job without poses: every valid job's bytes are the single
    call's, the bad job carries E_ARG, one launch per table plan and one wait"""
    from ndtpso_slam_amd import capi
    cases = [sc.device_case(ctx, cell_side=cs) for cs in (0.5, 0.3, 0.25)]
    poses = _poses()
    jobs = [(cases[0][0], cases[0][1], poses[:5]), (cases[1][0], cases[1][1], poses[3:9]), (cases[2][0], cases[2][1], poses[:1]),
            (cases[0][0], cases[1][1], poses[5:]),      # map 0 again, scan 1 again
            (cases[1][0], cases[0][1], np.zeros((0, 3))),
            (cases[2][0], cases[0][1], poses[17:18])]
    single = [m.curvature(s, p)["raw"].tobytes() if len(p) else None for m, s, p in jobs]
    out, stats = capi.curvature_maps(ctx, jobs)
    plans = set()
    for (cv, rc, route), want, job in zip(out, single, jobs):
        if want is None:
            assert rc == capi.E_ARG
            continue
        assert rc == capi.OK and route == 1
        assert cv["raw"].tobytes() == want
        plans.update(cv["path"].tolist())
    assert 1 <= stats["launches"] <= len(plans) and stats["waits"] == 1 and stats["single_jobs"] == 0, (stats, plans)
    one, st1 = capi.curvature_maps(ctx, jobs[:1])
    assert one[0][1] == capi.OK and one[0][2] == 0 and one[0][0]["raw"].tobytes() == single[0]     # a call of one job: route 0
    assert st1["single_jobs"] == 1 and st1["launches"] == 0
    # the raw call returns the first failing job's rc
    n = len(jobs)
    raw = (capi.MapCurvatureJob * n)()
    keep = []
    for j, (m, s, p) in zip(raw, jobs):
        p = np.ascontiguousarray(p, dtype=np.float64).reshape(-1, 3)
        rec = np.zeros(max(len(p), 1), dtype=capi.CURVATURE_DTYPE)
        buf = p if len(p) else np.zeros((1, 3))
        keep.append((buf, rec))
        j.map, j.new_points, j.n_poses = m._h, s._h, len(p)
        j.poses = buf.ctypes.data_as(C.POINTER(C.c_double))
        j.out = C.cast(rec.ctypes.data, C.POINTER(capi.Curvature))
    assert ctx._lib.ndtpso_map_curvature_batch(ctx._h, raw, n, None) == capi.E_ARG
    assert [j.rc for j in raw] == [0, 0, 0, 0, capi.E_ARG, 0]
    # refused as a whole, before anything is written: a null pointer, no jobs, too many poses in all
    assert ctx._lib.ndtpso_map_curvature_batch(ctx._h, None, 1, None) == capi.E_ARG
    assert ctx._lib.ndtpso_map_curvature_batch(ctx._h, raw, 0, None) == capi.E_ARG
    raw[0].rc = 77
    raw[1].n_poses = capi.CURVATURE_MAX_POSES
    assert ctx._lib.ndtpso_map_curvature_batch(ctx._h, raw, n, None) == capi.E_ARG and raw[0].rc == 77
    # a pose that is not finite is its job's error
    bad = [(cases[0][0], cases[0][1], poses[:2]), (cases[1][0], cases[1][1], [[0.0, float("nan"), 0.0]])]
    out, _ = capi.curvature_maps(ctx, bad)
    assert out[0][1] == capi.OK and out[1][1] == capi.E_ARG and out[0][0]["raw"].tobytes() == single[0][:2 * 96]


@pytest.mark.parametrize("pending", ["inserts", "speculation"])
def test_map_state_is_the_cost_calls(ctx, pending):
    """on a map with inserts and no build (or a pending speculative build) curvature builds (commits) as cost() does: the next
    align returns the bytes a twin map returns after cost() in its place"""
    from ndtpso_slam_amd import capi
    cfg = capi.PSOConfig.make(20, 16)
    got = []
    for call in ("curvature", "cost"):
        m, s = sc.device_case(ctx, build=False)
        if pending == "speculation":
            m.build()
            maps, query = sc.ranges()
            s.load_scan(maps[0], sc.geom(), clip=m.grid)
            m.insert(s, (0.5, 0.5, 0.1))
            m.speculate_build()
            s.load_scan(query, sc.geom(), clip=m.grid)
        else:
            assert m.info()["n_built"] == 0
        if call == "curvature":
            c = m.curvature(s, sc.TRUTH)["cost"]
        else:
            c = m.cost(s, sc.TRUTH, mode=capi.SCORE_F64)
        assert m.info()["n_built"] > 0
        pose, cost, _ = m.align(s, sc.TRUTH, (0.1, 0.1, 3.1415e-3), cfg, seed=5, mode=capi.SCORE_F64)
        got.append(c.tobytes() + pose.tobytes() + np.float64(cost).tobytes())
    assert got[0] == got[1]


def test_snapshot(ctx, case):
    from ndtpso_slam_amd import capi
    m, s = case
    poses = _poses()
    twin = capi.ResidentMap.restore(ctx, m.snapshot(), pool_bytes=64 << 20)
    assert twin.curvature(s, poses)["raw"].tobytes() == m.curvature(s, poses)["raw"].tobytes()


def _inverse(pose, q):
    """the scan point that `pose` takes to q"""
    c, s = math.cos(pose[2]), math.sin(pose[2])
    d = np.asarray(q) - pose[:2]
    return np.array([d[0] * c + d[1] * s, -d[0] * s + d[1] * c])


def test_special_terms(ctx):
    from ndtpso_slam_amd import capi
    m, s = sc.device_case(ctx, build=False)
    truth = np.array(sc.TRUTH)
    grid = (sc.FRAME_M, sc.FRAME_M, sc.CELL_SIDE)
    taken = {c["index"] for c in m.cells()}
    import np_ref
    tight_cell, nan_cell = np.array([20.0, 20.0]), np.array([21.0, 20.0])       # low corners of two cells far from the room
    for corner in (tight_cell, nan_cell):
        assert np_ref.cell_index(corner[0] + 0.1, corner[1] + 0.1, *grid) not in taken
    rng = np.random.default_rng(8)
    m.insert_host(tight_cell + 0.05 + rng.uniform(-5e-4, 5e-4, (6, 2)), (0, 0, 0))      # a Gaussian a millimetre wide
    m.insert_host(np.tile(nan_cell + (0.26, 0.23), (3, 1)), (0, 0, 0))                  # three coincident points: NaN inverse covariance
    m.build()
    xy = s.get()
    # a point 0.4 m from the tight cell's mean, inside the cell: Q / 2 is far beyond 745, e == +0.
    far = _inverse(truth, tight_cell + 0.45)
    with_far = capi.ResidentScan(ctx, len(xy) + 1)
    with_far.set(np.concatenate([xy, [far]]))
    a, b = m.curvature(s, truth), m.curvature(with_far, truth)
    assert b["n_hit"][0] == a["n_hit"][0] + 1 and b["n_points"][0] == a["n_points"][0] + 1
    assert np.isfinite(_ten(b, 0)).all()
    # 361 and 362 points are the same trips (a group of four chunks and two more): the point's share is exactly zero, so the bits stay
    assert _sum_bytes(a) == _sum_bytes(b)
    _check_parity(ctx, m, with_far, [truth], "e == 0")
    # a point in the coincident-points cell: cost NaN, all nine derivatives NaN
    with_nan = capi.ResidentScan(ctx, len(xy) + 1)
    with_nan.set(np.concatenate([xy, [_inverse(truth, nan_cell + (0.28, 0.24))]]))
    c = m.curvature(with_nan, truth)
    assert np.isnan(_ten(c, 0)).all() and c["n_hit"][0] == a["n_hit"][0] + 1
    assert np.isnan(m.cost(with_nan, truth, mode=capi.SCORE_F64)).all()
    assert not capi.curvature_covariance({"hessian": c["hessian"][0]})["definite"]


def _corridor(ctx, axis=0.0):
    """two parallel walls 2 m apart and 20 m long, 1 cm of noise across them, as map and as scan"""
    from ndtpso_slam_amd import capi
    rng = np.random.default_rng(21)
    t = np.linspace(-10.0, 10.0, 500)
    walls = np.concatenate([np.stack([t, np.full_like(t, 1.0)], axis=1), np.stack([t, np.full_like(t, -1.0)], axis=1)])
    walls[:, 1] += rng.normal(0, 0.01, len(walls))
    c, s = math.cos(axis), math.sin(axis)
    walls = np.stack([walls[:, 0] * c - walls[:, 1] * s, walls[:, 0] * s + walls[:, 1] * c], axis=1)
    m = capi.ResidentMap(ctx, capi.Grid(sc.FRAME_M, sc.FRAME_M, sc.CELL_SIDE))
    m.insert_host(walls, None)
    scan = capi.ResidentScan(ctx, len(walls))
    scan.set(walls)
    return m, scan


def test_it_means_something(ctx, case):
    """conditions from the geometry: in the furnished room the refined pose is a definite minimum; in a corridor the pose is
    definite too (the noise constrains it a little) but its translational uncertainty lies along the corridor and is far more
    elongated than the room's"""
    from ndtpso_slam_amd import capi
    m, s = case
    poses, costs, index, _ = m.search(s, sc.ORIGIN, sc.STEP, sc.COUNT, sc.TOP_K, mode=capi.SCORE_F64)
    cfg = capi.PSOConfig.make()
    refined, cost, _ = m.align(s, poses[0], tuple(v / 2 for v in sc.STEP), cfg, seed=7, mode=capi.SCORE_F64)
    assert np.hypot(*(refined[:2] - np.array(sc.TRUTH)[:2])) < 0.05
    room = capi.curvature_covariance({"hessian": m.curvature(s, refined)["hessian"][0]})
    assert room["definite"]
    for axis in (0.0, 0.6):
        cm, cs_ = _corridor(ctx, axis)
        cor = capi.curvature_covariance({"hessian": cm.curvature(cs_, (0.0, 0.0, 0.0))["hessian"][0]})
        print("room", room["xy_major"], room["xy_minor"], room["xy_angle"], "corridor", cor["xy_major"], cor["xy_minor"], cor["xy_angle"])
        assert cor["definite"]
        off = (cor["xy_angle"] - axis + math.pi / 2) % math.pi - math.pi / 2
        assert abs(off) < math.pi / 4
        assert cor["xy_major"] / cor["xy_minor"] > room["xy_major"] / room["xy_minor"]


# ---- the drop-in: NDTFrame::curvature / curvatureBatch through host/replay/curvature_check ---------------------------------------

N_SCANS, SEED = 12, 7


@pytest.fixture(scope="module")
def sequence(tmp_path_factory):
    """tests/test_gpu_fleet.py's recipe at this file's 361 beams"""
    from ndtpso_slam_amd import synth
    rng = np.random.default_rng(4)
    t = np.linspace(0.0, 0.9, N_SCANS)
    poses = np.stack([2.0 + 1.2 * t, -1.0 + 0.8 * np.sin(1.5 * t), 0.3 + 0.25 * t], axis=1)
    clean = synth.raycast(poses, sc.N_BEAMS, synth.ANGLE_MIN, sc.angle_inc())
    ranges = np.where(clean > 0, clean + rng.normal(0, 0.01, clean.shape), 0.0).astype(np.float32)
    path = tmp_path_factory.mktemp("curvature") / "scans.bin"
    with open(path, "wb") as f:
        np.array([N_SCANS, sc.N_BEAMS], dtype=np.int32).tofile(f)
        np.array([synth.ANGLE_MIN, sc.angle_inc(), synth.RANGE_MAX], dtype=np.float32).tofile(f)
        ranges.tofile(f)
    return path, ranges


def _env():
    env = {k: v for k, v in os.environ.items() if k not in ("NDTPSO_SCORE", "NODE_FLEET_SEQUENTIAL")}
    env["NDTPSO_SCORE"] = "f64"
    return env


def _tool(args):
    r = subprocess.run([os.path.join(HOST, "replay", "curvature_check")] + [str(a) for a in args], text=True, capture_output=True,
                       env=_env(), timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return r.stdout.splitlines()


def test_drop_in_member(ctx, sequence):
    """every curvature curvature_check prints equals ResidentMap.curvature on a Python replay of the sequence, byte for byte, and
    its pose log is node_replay's without any curvature call: it draws nothing from rand() and leaves the tracking state alone"""
    from ndtpso_slam_amd import capi
    path, ranges = sequence
    common = [path, sc.FRAME_M, sc.CELL_SIDE, 50, 30, SEED]
    lines = _tool(["member"] + common)
    pose_log = "".join(l[len("pose 0 "):] + "\n" for l in lines if l.startswith("pose 0 "))
    replay = subprocess.check_output([os.path.join(HOST, "replay", "node_replay")] + [str(a) for a in common], env=_env(), text=True)
    assert pose_log == replay
    curv = [l.split() for l in lines if l.startswith("curv ")]
    assert len(curv) == N_SCANS - 1 and [int(w[2]) for w in curv] == list(range(1, N_SCANS))
    # the Python replay: the node's calls on a resident map, at the poses the tool aligned to
    grid = capi.Grid(sc.FRAME_M, sc.FRAME_M, sc.CELL_SIDE)
    one_cell = capi.Grid(sc.FRAME_M, sc.FRAME_M, float(sc.FRAME_M))
    ref = capi.ResidentMap(ctx, grid)
    s = capi.ResidentScan(ctx, sc.N_BEAMS)
    # (scan 0 arrives in a frame with cells of its own: its points reach the map in that frame's cell order)
    first = capi.ResidentMap(ctx, grid)
    s.load_scan(ranges[0], sc.geom(), trans=(0.0, 0.0, 0.0))
    first.insert(s, None)
    ref.insert_host(first.points(slot0_only=True), (0.0, 0.0, 0.0))
    for w in curv:
        k = int(w[2])
        vals = [float.fromhex(v) for v in w[3:16]]
        pose = np.array(vals[:3])
        s.load_scan(ranges[k], sc.geom(), trans=(0.0, 0.0, 0.0), clip=one_cell)
        cv = ref.curvature(s, pose)
        got = np.array(vals[3:])
        assert got.tobytes() == _ten(cv, 0).tobytes(), (k, got, _ten(cv, 0))
        assert [int(w[16]), int(w[17])] == [int(cv["n_points"][0]), int(cv["n_hit"][0])]
        ref.insert(s, pose)


def test_drop_in_batch(sequence):
    """curvature_check batch 4 prints the bytes of four member runs, one per robot of the same fleet"""
    path, _ = sequence
    common = [path, sc.FRAME_M, sc.CELL_SIDE, 50, 30, SEED]
    batch = _tool(["batch", 4] + common)
    assert sum(l.startswith("curv ") for l in batch) == 4 * (N_SCANS - 1)
    for r in range(4):
        member = _tool(["member"] + common + [4, r])
        assert member == [l for l in batch if l.split()[1] == str(r)], r
