"""ndtpso_map_trace / ndtpso_map_trace_batch / ndtpso_map_get_nav_grid on the device: the counters against the restatement of the
contract (tests/trace_ref.py, with the device's own sincos), at the launch's edges, on hand-made rays, alone and in batches, in any
order, as an observer of everything else a map does, through its lifecycle, and through the drop-in (NDTFrame::setTraceOnUpdate /
traceCounts / navGrid).  Scans come from tests/search_case.py: 361 beams of the synthetic room, a 60 m frame, og_cell_size 0.25
(a 240 x 240 grid, rays of some tens of cells).  Every comparison of counters is np.array_equal: there is nothing to tolerate."""
import math
import os
import subprocess

import numpy as np
import pytest

import search_case as sc
import trace_ref as tr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "host")
OG = 0.25
SEVEN = list(sc.MAP_POSES) + [sc.TRUTH]


def _map(ctx, og=OG, frame=sc.FRAME_M, cell_side=sc.CELL_SIDE, height=None):
    from ndtpso_slam_amd import capi
    return capi.ResidentMap(ctx, capi.Grid(frame, height or frame, cell_side), og_cell_size=og, pool_bytes=64 << 20)


def _sincos(ctx, theta):
    sn, cn = ctx.device_math("sincos", [theta])
    return float(cn[0]), float(sn[0])


def _ref(ctx, traces, og=OG, frame=sc.FRAME_M):
    """the restatement's counters of `traces` = [(xy, pose), ...]"""
    cnt = tr.Counters(frame, frame, og)
    for xy, pose in traces:
        cnt.trace(xy, pose, *_sincos(ctx, pose[2]))
    return cnt


def _check(m, cnt, what=""):
    hits, passes = m.trace_counts()
    info = m.trace_info()
    want_hits, want_passes = cnt.grids()
    print(what, "rays", info["n_rays"], "skipped", info["n_skipped"], "steps", info["n_steps"], "extent", info["extent"])
    assert hits.dtype == np.uint32 and passes.dtype == np.uint64 and hits.shape == passes.shape == (cnt.h, cnt.w)
    assert np.array_equal(hits, want_hits), (what, np.argwhere(hits != want_hits)[:5])
    assert np.array_equal(passes, want_passes), (what, np.argwhere(passes != want_passes)[:5])
    assert (info["n_rays"], info["n_skipped"], info["n_steps"]) == (cnt.n_rays, cnt.n_skipped, cnt.n_steps), what
    if cnt.n_rays:
        assert list(info["extent"]) == cnt.extent, what
    assert info["allocated"] == 1 and (info["width"], info["height"]) == (cnt.w, cnt.h)
    return hits, passes, info


@pytest.fixture(scope="module")
def scans(ctx):
    """the six map scans and the query as device-resident scans, with their points as the device holds them"""
    from ndtpso_slam_amd import capi
    maps, query = sc.ranges()
    grid = capi.Grid(sc.FRAME_M, sc.FRAME_M, sc.CELL_SIDE)
    out = []
    for r in list(maps) + [query]:
        s = capi.ResidentScan(ctx, sc.N_BEAMS)
        s.load_scan(r, sc.geom(), clip=grid)
        xy = s.get()
        xy.setflags(write=False)
        out.append((s, xy))
    return out


@pytest.fixture(scope="module")
def seven(ctx, scans):
    """the restatement's counters of the seven traces, computed once"""
    return _ref(ctx, [(xy, pose) for (_, xy), pose in zip(scans, SEVEN)])


@pytest.fixture(scope="module")
def room(ctx, scans, seven):
    """a built map of the six scans with the seven traces in it"""
    m = _map(ctx)
    for (s, _), pose in zip(scans[:6], sc.MAP_POSES):
        m.insert(s, pose)
    m.build()
    for (s, _), pose in zip(scans, SEVEN):
        m.trace(s, pose)
    return m


@pytest.fixture()
def blank(ctx):
    """a map nothing was done to, for one test"""
    m = _map(ctx)
    yield m
    m.close()


def test_parity(room, seven):
    hits, passes, info = _check(room, seven, "parity")
    assert hits.sum() == info["n_rays"] == seven.n_rays > 6 * sc.N_BEAMS          # (the room returns nearly every beam)
    assert passes.sum() == info["n_steps"] == seven.n_steps > 20 * info["n_rays"]  # rays of some tens of cells
    assert info["n_skipped"] == 0


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257])
def test_ray_counts_at_the_launch_edges(ctx, scans, blank, n):
    from ndtpso_slam_amd import capi
    xy = scans[6][1]
    p = capi.ResidentScan(ctx, max(n, 1))
    p.set(xy[:n])
    blank.trace(p, sc.TRUTH)
    hits, passes, info = _check(blank, _ref(ctx, [(xy[:n], sc.TRUTH)]), "n = %d" % n)
    assert hits.sum() == info["n_rays"] == n


C0 = (0.125, 0.125)    # the centre of cell (120, 120)


def _hand_cases():
    cs = OG
    diag = [[sx * 2 * cs, sy * 2 * cs] for sx in (1, -1) for sy in (1, -1)]
    return {
        "dx == 0, dy == 0, zero length": ([[0.0, 1.3], [0.0, -2.1], [1.7, 0.0], [-0.9, 0.0], [0.0, 0.0]], (C0[0], C0[1], 0.0)),
        "four signs": ([[3.1, 1.2], [-3.1, 1.2], [3.1, -1.2], [-3.1, -1.2], [0.3, 7.7], [-0.3, -7.7]], (0.4, -0.3, 0.0)),
        "exact corners: ties": (diag + [[3 * cs, 3 * cs], [-5 * cs, 5 * cs], [4 * cs, -4 * cs]], (C0[0], C0[1], 0.0)),
        "ends on a border": ([[0.375, 0.0], [0.375, 0.375], [-0.125, 0.0], [0.0, -0.125], [2.375, 1.125]], (C0[0], C0[1], 0.0)),
        "at and beyond the bound": ([[29.875, 0.0], [29.874, 0.0], [40.0, 0.0], [0.0, -29.875 - 0.25], [0.0, 29.8], [-30.125, 0.0]],
                                    (C0[0], C0[1], 0.0)),
        "origin on the bound": ([[1.0, 0.0], [0.0, 1.0]], (30.0, 0.0, 0.0)),
        "origin beyond the bound": ([[-35.0, 0.0]], (31.0, 0.0, 0.0)),
        "turned": ([[3.1, 1.2], [-3.1, 1.2], [0.0, 5.0], [6.0, 0.0], [2 * cs, 2 * cs]], (C0[0], C0[1], 0.45)),
        "a heading of 7 rad": ([[3.1, 1.2], [-3.1, 1.2], [0.0, 5.0], [6.0, 0.0], [10.0, -4.0]], (-1.0, 2.0, 7.0)),
    }


@pytest.mark.parametrize("name", list(_hand_cases()))
def test_hand_made_rays(ctx, blank, name):
    from ndtpso_slam_amd import capi
    xy, pose = _hand_cases()[name]
    xy = np.array(xy, dtype=np.float64)
    p = capi.ResidentScan(ctx, len(xy))
    p.set(xy)
    blank.trace(p, pose)
    cnt = _ref(ctx, [(xy, pose)])
    hits, passes, info = _check(blank, cnt, name)
    if name.startswith("dx == 0"):
        assert hits[120, 120] == 1 and passes[120, 120] == 4           # the zero-length ray: one hit in the origin's cell, no pass
        assert hits[125, 120] == 1 and passes[121:125, 120].tolist() == [1] * 4 and passes[:, 121].sum() == passes[120, 121] == 1
    if name.startswith("exact corners"):
        for sx in (1, -1):                                               # x steps first on every tie
            for sy in (1, -1):
                assert passes[120, 120 + sx] >= 1 and passes[120 + sy, 120] == 0, (sx, sy)
        assert info["n_steps"] == 4 * 4 + 6 + 10 + 8
    if name.startswith("ends on a border"):
        assert hits[120, 122] == 1 and hits[122, 122] == 1 and hits[120, 120] == 2 and hits[125, 130] == 1
    if name.startswith("at and beyond"):
        assert (info["n_rays"], info["n_skipped"]) == (2, 4) and hits[120, 239] == 1 and hits[239, 120] == 1
    if name.startswith("origin"):
        assert (info["n_rays"], info["n_skipped"]) == (0, len(xy)) and not hits.any() and not passes.any()   # nothing written
        assert info["extent"] == (0xffffffff, 0, 0xffffffff, 0)


def _bytes(m):
    hits, passes = m.trace_counts()
    info = m.trace_info()
    return hits.tobytes() + passes.tobytes() + repr(sorted(info.items())).encode()


def test_batch(ctx, scans):
    """jobs over three maps, a map named three times, a scan named twice, one job refused: every map's counters are byte for byte
    those of the single calls on twin maps"""
    from ndtpso_slam_amd import capi
    ogs = (0.25, 0.5, 0.1)
    maps, twins = [_map(ctx, og) for og in ogs], [_map(ctx, og) for og in ogs]
    no_grid = _map(ctx, 0.0)
    plan = [(0, 0, SEVEN[0]), (1, 1, SEVEN[1]), (0, 2, SEVEN[2]), (2, 3, SEVEN[3]), (0, 2, SEVEN[4]), (1, 6, SEVEN[6]), (2, 5, SEVEN[5])]
    jobs = [(maps[a], scans[b][0], pose) for a, b, pose in plan]
    jobs.insert(3, (no_grid, scans[0][0], SEVEN[0]))
    jobs.insert(5, (maps[1], scans[0][0], (0.0, float("nan"), 0.0)))
    rcs = capi.trace_maps(ctx, jobs)
    assert rcs == [0, 0, 0, capi.E_STATE, 0, capi.E_ARG, 0, 0, 0]
    for a, b, pose in plan:
        twins[a].trace(scans[b][0], pose)
    for m, t, og in zip(maps, twins, ogs):
        assert _bytes(m) == _bytes(t), og
        assert m.trace_info()["n_rays"] > 0
    assert no_grid.trace_info()["allocated"] == 0
    # against the restatement too, on the coarse map (its counters were filled by the batch alone)
    _check(maps[1], _ref(ctx, [(scans[1][1], SEVEN[1]), (scans[6][1], SEVEN[6])], og=0.5), "batch, og 0.5")
    # the call's own refusals write nothing: not a job's rc, not a counter
    before = [_bytes(m) for m in maps]
    other = capi.Context(0)
    try:
        foreign_scan = capi.ResidentScan(other, 4)
        foreign_map = capi.ResidentMap(other, capi.Grid(20, 20, 1.0), og_cell_size=0.5)
        arr = (capi.MapTraceJob * 2)()
        for j in arr:
            j.map, j.points, j.rc = maps[0]._h, scans[0][0]._h, 77
            j.pose[:] = [0.0, 0.0, 0.0]
        L = ctx._lib
        assert L.ndtpso_map_trace_batch(ctx._h, arr, 0) == capi.E_ARG
        assert L.ndtpso_map_trace_batch(ctx._h, None, 2) == capi.E_ARG
        arr[1].points = None
        assert L.ndtpso_map_trace_batch(ctx._h, arr, 2) == capi.E_ARG
        arr[1].points = foreign_scan._h
        assert L.ndtpso_map_trace_batch(ctx._h, arr, 2) == capi.E_ARG
        arr[1].points, arr[1].map = scans[0][0]._h, foreign_map._h
        assert L.ndtpso_map_trace_batch(ctx._h, arr, 2) == capi.E_ARG
        assert [j.rc for j in arr] == [77, 77]
        with pytest.raises(capi.NdtpsoError) as e:
            maps[0].trace(foreign_scan, (0.0, 0.0, 0.0))
        assert e.value.code == capi.E_ARG
        with pytest.raises(capi.NdtpsoError) as e:
            maps[0].trace(scans[0][0], (0.0, 0.0, float("inf")))
        assert e.value.code == capi.E_ARG
        assert L.ndtpso_map_trace(maps[0]._h, scans[0][0]._h, None) == capi.E_ARG
        foreign_scan.close()
        foreign_map.close()
    finally:
        other.close()
    assert [_bytes(m) for m in maps] == before


def test_order_and_grouping_do_not_matter(ctx, scans, room, seven):
    from ndtpso_slam_amd import capi
    want = room.trace_counts()
    jobs = lambda m: [(m, s, pose) for (s, _), pose in zip(scans, SEVEN)]
    rev, split, one = _map(ctx), _map(ctx), _map(ctx)
    for (s, _), pose in reversed(list(zip(scans, SEVEN))):
        rev.trace(s, pose)
    assert capi.trace_maps(ctx, jobs(split)[:3]) == [0] * 3 and capi.trace_maps(ctx, jobs(split)[3:]) == [0] * 4
    assert capi.trace_maps(ctx, jobs(one)) == [0] * 7
    for m in (rev, split, one):
        got = m.trace_counts()
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        info = m.trace_info()
        assert (info["n_rays"], info["n_steps"], list(info["extent"])) == (seven.n_rays, seven.n_steps, seven.extent)


def test_observer(ctx, scans):
    """twin maps through inserts, speculate_build, align (exact), cost, curvature, search and snapshot; on one of them a trace between
    every two steps, the one between speculate_build and the align that commits it included: every result is byte-identical, and a
    map's snapshot is the same blob before and after a trace"""
    from ndtpso_slam_amd import capi
    cfg = capi.PSOConfig.make(20, 12)
    q = scans[6][0]
    poses = capi.lattice_poses(sc.ORIGIN, sc.STEP, sc.COUNT)[::97]

    def run(traced):
        m = _map(ctx)
        out = []
        k = [0]

        def trace():
            if traced:
                m.trace(scans[k[0] % 7][0], SEVEN[k[0] % 7])
                k[0] += 1
        trace()
        for i in range(3):
            m.insert(scans[i][0], sc.MAP_POSES[i])
            trace()
        m.speculate_build()
        trace()
        pose, cost, st = m.align(q, (1.25, -0.65, 0.44), (0.15, 0.15, 0.03), cfg, seed=5, mode=capi.SCORE_EXACT)
        out += [pose.tobytes(), np.float64(cost).tobytes()]
        trace()
        m.insert(scans[3][0], sc.MAP_POSES[3])
        m.speculate_build()
        trace()
        out.append(m.cost(q, poses, mode=capi.SCORE_F64).tobytes())
        trace()
        out.append(m.curvature(q, [sc.TRUTH])["raw"].tobytes())
        trace()
        hp, hc, hi, _ = m.search(q, sc.ORIGIN, sc.STEP, sc.COUNT, sc.TOP_K, mode=capi.SCORE_EXACT)
        out += [hp.tobytes(), hc.tobytes(), hi.tobytes()]
        trace()
        m.insert(scans[4][0], sc.MAP_POSES[4])
        m.speculate_build()
        trace()                                  # (a speculation is pending: the snapshot puts it back)
        blob = m.snapshot()
        # (twin maps list their created cells in the order their inserts' atomics landed -- ndtpso_map_snapshot.inc -- so the twins'
        # blobs are compared by what they hold, and byte for byte on the SAME map around a trace)
        out.append(repr(sorted((k, v) for k, v in capi.snapshot_describe(blob).items())).encode())
        trace()
        if traced:
            assert m.snapshot() == blob
        out.append(repr([(c["index"], c["count"], c["built"], c["slot"], c["mean"].tobytes(), c["icov"].tobytes()) for c in m.cells()]).encode())
        out.append(m.points().tobytes())
        og = m.occupancy()
        out.append(og[0].tobytes() + repr(og[1:]).encode())
        out.append(repr(sorted(m.info().items())).encode())
        n_traced = m.trace_info()["n_rays"]
        m.close()
        return out, n_traced

    plain, n0 = run(False)
    traced, n1 = run(True)
    assert n0 == 0 and n1 > 10 * sc.N_BEAMS
    assert len(plain) == len(traced)
    for i, (a, b) in enumerate(zip(plain, traced)):
        assert a == b, i


def test_nav_grid(ctx, scans, room, seven):
    nav = room.nav_grid()
    og, w, h, _ = room.occupancy()
    hits, passes = room.trace_counts()
    occ = og.reshape(h, w)
    assert nav.dtype == np.int8 and nav.shape == (h, w)
    assert np.array_equal(nav, tr.nav_grid(occ, hits, passes))
    assert (occ > 0).any() and (nav == 0).sum() > 1000 and (nav == -1).sum() > 1000 and nav.min() == -1 and nav.max() <= 100
    # from TRUTH along a beam that ends on the room's outer wall (x = +-12 or y = +-9: nothing looks behind it)
    xy = scans[6][1]
    cn, sn = _sincos(ctx, sc.TRUTH[2])
    ends = tr.end_points(xy, sc.TRUTH, cn, sn)
    o = np.array(sc.TRUTH[:2])
    dirs = (ends - o) / np.linalg.norm(ends - o, axis=1)[:, None]
    on_x, on_y = np.abs(ends[:, 0]) > 11.9, np.abs(ends[:, 1]) > 8.9
    square_on = np.where(on_x, np.abs(dirs[:, 0]), np.where(on_y, np.abs(dirs[:, 1]), 0.0))   # the beam that meets it most squarely
    b = int(np.argmax(square_on))
    e, u = ends[b], dirs[b]
    length = float(np.linalg.norm(e - o))
    assert length > 5.0 and square_on[b] > 0.95
    cells = tr.ray_cells((float(o[0]), float(o[1])), (float(e[0]), float(e[1])), 30.0, 30.0, OG)
    cell_of = lambda q: (int(math.floor((q[0] + 30.0) / OG)), int(math.floor((q[1] + 30.0) / OG)))
    # before the wall (more than two map cells short of it): free.  The reference rasterises a Gaussian inside its own built map
    # cell only, built cells lie on the walls and the four boxes, and the beams that meet an outer wall squarely from TRUTH run
    # more than two metres clear of every box: no cell of this beam carries a word of the reference's, every one is 0.
    before = [(cx, cy) for cx, cy in cells if float(((np.array([cx, cy]) + 0.5) * OG - 30.0 - o) @ u) < length - 1.0]
    assert len(before) >= 10
    for cx, cy in before:
        assert occ[cy, cx] == 0 and nav[cy, cx] == 0 and hits[cy, cx] == 0 and passes[cy, cx] >= 1, (cx, cy)
    # the wall: the reference's value wherever that is > 0 (a thin wall on a cell border leaves the reference's grid at 0 on
    # either side: there the beams that ended in the cell speak)
    wall = [cell_of(e + d * u) for d in np.arange(-0.5, 0.51, 0.125)]
    for cx, cy in wall:
        if occ[cy, cx] > 0:
            assert nav[cy, cx] == occ[cy, cx]
    ex, ey = cells[-1]
    assert hits[ey, ex] >= 1 and nav[ey, ex] > 0
    # behind the wall (beyond the map cell the wall's points can fall into): unknown
    for d in np.arange(1.0, 3.01, 0.125):
        cx, cy = cell_of(e + d * u)
        assert nav[cy, cx] == -1 and hits[cy, cx] == 0 and passes[cy, cx] == 0, (d, cx, cy)


def test_lifecycle(ctx, scans):
    from ndtpso_slam_amd import capi
    s, xy = scans[2]
    pose = SEVEN[2]
    m = _map(ctx)
    info = m.trace_info()
    assert info["allocated"] == 0 and (info["width"], info["height"]) == (240, 240) and info["n_rays"] == 0
    hits, passes = m.trace_counts()                       # never traced: zeros
    assert hits.shape == (240, 240) and not hits.any() and not passes.any()
    assert (m.nav_grid() == -1).all()
    m.insert(s, pose)
    m.trace(s, pose)
    once = _bytes(m)
    assert m.trace_info()["n_rays"] > 300
    m.reset()                                             # resetCells keeps the counters
    assert _bytes(m) == once
    blob = m.snapshot()
    m.clear()                                             # clear zeroes counters and totals
    info = m.trace_info()
    assert info["allocated"] == 1 and (info["n_rays"], info["n_skipped"], info["n_steps"]) == (0, 0, 0)
    assert info["extent"] == (0xffffffff, 0, 0xffffffff, 0)
    hits, passes = m.trace_counts()
    assert not hits.any() and not passes.any()
    m.trace(s, pose)
    assert _bytes(m) == once
    # a restored snapshot starts with no counters; tracing it equals tracing a fresh twin
    r = capi.ResidentMap.restore(ctx, blob, pool_bytes=64 << 20)
    assert r.trace_info()["allocated"] == 0 and not r.trace_counts()[0].any()
    r.trace(s, pose)
    assert _bytes(r) == once
    # refusals: a grid that is not square, a map without an occupancy grid
    wide = _map(ctx, frame=60, height=40)
    with pytest.raises(capi.NdtpsoError) as e:
        wide.trace(s, pose)
    assert e.value.code == capi.E_ARG and wide.trace_info()["allocated"] == 0
    none = _map(ctx, og=0.0)
    with pytest.raises(capi.NdtpsoError) as e:
        none.trace(s, pose)
    assert e.value.code == capi.E_STATE
    with pytest.raises(capi.NdtpsoError) as e:
        none.nav_grid()
    assert e.value.code == capi.E_STATE
    empty = capi.ResidentScan(ctx, 4)                     # an empty scan is no error
    m.trace(empty, pose)
    assert _bytes(m) == once


def test_workload_shape(ctx):
    """1081 beams, og_cell_size 0.05, a 60 m frame, one scan: the totals against a vectorised count of nx + ny per ray"""
    from ndtpso_slam_amd import capi, synth
    pose = (1.3, -0.7, 0.45)
    clean = synth.raycast(np.asarray(pose)[None, :])[0]
    ranges = np.where(clean > 0, clean + np.random.default_rng(3).normal(0, 0.01, clean.shape), 0.0).astype(np.float32)
    geom = capi.ScanGeom(synth.N_BEAMS, synth.ANGLE_MIN, synth.ANGLE_INC, synth.RANGE_MAX, 0.1)
    m = _map(ctx, og=0.05)
    s = capi.ResidentScan(ctx, synth.N_BEAMS)
    s.load_scan(ranges, geom, clip=m.grid)
    m.trace(s, pose)
    n_rays, n_skipped, n_steps = tr.steps_of(s.get(), pose, *_sincos(ctx, pose[2]), 60, 60, 0.05)
    hits, passes = m.trace_counts()
    info = m.trace_info()
    print("rays", n_rays, "steps", n_steps, "steps per ray", n_steps / max(n_rays, 1))
    assert (info["n_rays"], info["n_skipped"], info["n_steps"]) == (n_rays, n_skipped, n_steps)
    assert hits.sum() == n_rays > 1000 and passes.sum() == n_steps > 100 * n_rays


# ---- the drop-in: NDTFrame::setTraceOnUpdate / traceCounts / navGrid through host/replay/trace_check -------------------------------

N_SCANS, SEED = 12, 7


@pytest.fixture(scope="module")
def sequence(tmp_path_factory):
    """tests/test_gpu_map_curvature.py's recipe"""
    from ndtpso_slam_amd import synth
    rng = np.random.default_rng(4)
    t = np.linspace(0.0, 0.9, N_SCANS)
    poses = np.stack([2.0 + 1.2 * t, -1.0 + 0.8 * np.sin(1.5 * t), 0.3 + 0.25 * t], axis=1)
    clean = synth.raycast(poses, sc.N_BEAMS, synth.ANGLE_MIN, sc.angle_inc())
    ranges = np.where(clean > 0, clean + rng.normal(0, 0.01, clean.shape), 0.0).astype(np.float32)
    d = tmp_path_factory.mktemp("trace")
    with open(d / "scans.bin", "wb") as f:
        np.array([N_SCANS, sc.N_BEAMS], dtype=np.int32).tofile(f)
        np.array([synth.ANGLE_MIN, sc.angle_inc(), synth.RANGE_MAX], dtype=np.float32).tofile(f)
        ranges.tofile(f)
    return d, ranges


def _env():
    env = {k: v for k, v in os.environ.items() if k not in ("NDTPSO_SCORE", "NODE_FLEET_SEQUENTIAL", "NDTPSO_ABORT_ON_ERROR")}
    env["NDTPSO_SCORE"] = "f64"
    return env


def _tool(exe, args):
    r = subprocess.run([os.path.join(HOST, "replay", exe)] + [str(a) for a in args], text=True, capture_output=True, env=_env(), timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return r.stdout


def _files(prefix, r=0):
    return tuple(np.fromfile("%s.%d.%s" % (prefix, r, ext), dtype=dt) for ext, dt in (("hits", np.uint32), ("passes", np.uint64), ("nav", np.int8)))


def _python_replay(ctx, ranges, order, log):
    """the node's calls on a resident map with capi, every scan inserted and traced at the pose the tool logged for it"""
    from ndtpso_slam_amd import capi
    grid = capi.Grid(sc.FRAME_M, sc.FRAME_M, sc.CELL_SIDE)
    one_cell = capi.Grid(sc.FRAME_M, sc.FRAME_M, float(sc.FRAME_M))
    ref = capi.ResidentMap(ctx, grid, og_cell_size=OG)
    s = capi.ResidentScan(ctx, sc.N_BEAMS)
    for k, (src, pose) in enumerate(zip(order, log)):
        if k == 0:   # (scan 0 arrives in a frame with cells of its own: its points reach the map in that frame's cell order)
            first = capi.ResidentMap(ctx, grid)
            s.load_scan(ranges[src], sc.geom(), trans=(0.0, 0.0, 0.0))
            first.insert(s, None)
            pts = first.points(slot0_only=True)
            ref.insert_host(pts, pose)
            s.set(pts)
        else:
            s.load_scan(ranges[src], sc.geom(), trans=(0.0, 0.0, 0.0), clip=one_cell)
            ref.insert(s, pose)
        ref.trace(s, pose)
        if k + 1 < len(log):
            ref.build()      # (the next scan's align() builds the map first: the occupancy grid the nav grid overlays)
    hits, passes = ref.trace_counts()
    return hits.ravel(), passes.ravel(), ref.nav_grid().ravel()


def _log(out, r=0):
    return [tuple(float(v) for v in l.split()[3:6]) for l in out.splitlines() if l.startswith("pose %d " % r)]


def test_drop_in(ctx, sequence):
    d, ranges = sequence
    common = [d / "scans.bin", sc.FRAME_M, sc.CELL_SIDE, OG, 50, 30, SEED]
    on = _tool("trace_check", common + [d / "on"])
    off = _tool("trace_check", ["--no-trace"] + common + [d / "off"])
    host = _tool("trace_check", ["--host-trace"] + common + [d / "host"])
    assert on == off == host and len(_log(on)) == N_SCANS               # the pose log does not know about tracing
    replay = _tool("node_replay", [common[0], sc.FRAME_M, sc.CELL_SIDE, 50, 30, SEED])
    assert "".join(l[len("pose 0 "):] + "\n" for l in on.splitlines()) == replay
    assert not os.path.exists("%s.0.hits" % (d / "off"))
    got, walked = _files(d / "on"), _files(d / "host")
    want = _python_replay(ctx, ranges, range(N_SCANS), _log(on))
    assert got[0].sum() > 11 * 300
    for a, b, c, what in zip(got, walked, want, ("hits", "passes", "nav")):
        assert np.array_equal(a, c), what                                # capi's, for the same traces
        assert np.array_equal(a, b), what                                # the host's walk of the same rule


def test_drop_in_update_batch(ctx, sequence):
    """two robots in lock step: their traces leave through updateBatch's one ndtpso_map_trace_batch"""
    d, ranges = sequence
    common = [d / "scans.bin", sc.FRAME_M, sc.CELL_SIDE, OG, 50, 30, SEED]
    out = _tool("trace_check", common + [d / "fleet", 2])
    stride = N_SCANS // 2
    for r in range(2):
        order = [(r * stride + k) % N_SCANS for k in range(N_SCANS)]
        got = _files(d / "fleet", r)
        want = _python_replay(ctx, ranges, order, _log(out, r))
        assert got[0].sum() > 11 * 300
        for a, c, what in zip(got, want, ("hits", "passes", "nav")):
            assert np.array_equal(a, c), (r, what)


def _refusals(env):
    r = subprocess.run([os.path.join(HOST, "replay", "trace_check"), "--refusals"], text=True, capture_output=True, env=env, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    out = {}
    for l in r.stdout.splitlines():
        if l.startswith("refused "):
            head, _, text = l.partition(" -> ")
            _, frame, call, errors, ret = head.split()
            out[(frame, call)] = (int(errors), int(ret), text)
    assert len(out) == 5 * 4
    return out


def test_drop_in_refusals():
    """frames that cannot be traced are refused and the refusal is recorded (ndtpso_slam/status.h): a one-cell per-scan frame, a
    frame of 2.25 M cells, a frame without an occupancy grid or with one that is not square, and any frame under NDTPSO_RESIDENT=0"""
    env = {k: v for k, v in _env().items() if k != "NDTPSO_RESIDENT"}
    got = _refusals(env)
    for frame, why in (("one-cell", "a one-cell scan frame holds no map"), ("large", "a frame of 2^21 cells or more is kept on the host's side")):
        for call, what in (("traceFreeSpace", "traceFreeSpace: "), ("update", "update: trace: "), ("navGrid", "navGrid: "), ("traceCounts", "traceCounts: ")):
            errors, ret, text = got[(frame, call)]
            assert errors == 1 and ret in (-1, 0) and what + why in text, (frame, call, got[(frame, call)])
    for frame in ("no-grid", "not-square"):       # the C-ABI's own refusals (NDTPSO_E_STATE / NDTPSO_E_ARG), recorded by the drop-in
        assert got[(frame, "traceFreeSpace")][0] == 1 and "traceFreeSpace" in got[(frame, "traceFreeSpace")][2], got[(frame, "traceFreeSpace")]
        assert got[(frame, "update")][0] == 1 and "update: trace" in got[(frame, "update")][2], got[(frame, "update")]
        assert got[(frame, "traceCounts")][:2] == (0, 1)          # (zeros: nothing was traced)
    assert got[("no-grid", "navGrid")][:2] == (1, 0) and "navGrid" in got[("no-grid", "navGrid")][2]
    assert got[("not-square", "navGrid")][:2] == (0, 1)           # the grid can be formed, only tracing collides
    for call in ("traceFreeSpace", "update", "navGrid", "traceCounts"):
        assert got[("plain", call)][0] == 0 and got[("plain", call)][1] in (-1, 1), got[("plain", call)]
    off = _refusals(dict(env, NDTPSO_RESIDENT="0"))
    for frame in ("plain", "no-grid", "not-square"):
        for call, what in (("traceFreeSpace", "traceFreeSpace: "), ("update", "update: trace: "), ("navGrid", "navGrid: "), ("traceCounts", "traceCounts: ")):
            errors, ret, text = off[(frame, call)]
            assert errors == 1 and ret in (-1, 0) and what + "the frame is not resident" in text, (frame, call, off[(frame, call)])
