"""ndtpso_points_load_scans / ndtpso_map_update_batch (capi.load_scans / capi.update_maps): the scan loads and the map updates of
several single calls in shared launches (k_scans_to_resident_jobs, k_map_insert_jobs, k_map_build_jobs, k_map_pack_jobs).

The contract is the single calls': afterwards every scan and every map is bit for bit what ndtpso_points_load_scan, and
ndtpso_map_mark_unbuilt + ndtpso_map_insert [+ ndtpso_map_speculate_build], made in job order leave.  So every test drives TWIN
objects: one set of maps and scans through the batch entries, an identical set through the single calls, and compares what the
library lets a caller see -- ResidentScan.get(), ResidentMap.cells(), points() in window order and slot 0 alone, the header --
with array_equal / ==, never with a tolerance, and the alignments that follow (their path depends on the host's bookkeeping:
late window binding).  Inspecting a map takes a pending speculative build back, on both twins alike; the alignments between the
steps are what runs behind speculative builds that were left alone."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
DEV = (0.1, 0.1, 3.1415e-3)
INFO = ("n_created", "n_built", "status", "n_words", "x0", "x1", "y0", "y1", "n_points")


def _geom(n_beams=None):
    from ndtpso_slam_amd import capi, synth
    if n_beams is None:
        return capi.ScanGeom(synth.N_BEAMS, synth.ANGLE_MIN, synth.ANGLE_INC, synth.RANGE_MAX, 0.1)
    return capi.ScanGeom(n_beams, synth.ANGLE_MIN, np.float32(4.712389 / float(n_beams - 1)), synth.RANGE_MAX, 0.1)


def _rel(p0, p):
    c, s = np.cos(p0[2]), np.sin(p0[2])
    dx, dy = p[0] - p0[0], p[1] - p0[1]
    return np.array([c * dx + s * dy, -s * dx + c * dy, p[2] - p0[2]])


def _trajectory(n_scans, start, seed, step=0.6, n_beams=None):
    """(ranges [n, beams] with 1 cm noise, poses in scan 0's frame) along a short arc from `start`"""
    from ndtpso_slam_amd import synth
    rng = np.random.default_rng(seed)
    s = np.linspace(0.0, step, n_scans)
    poses = np.stack([start[0] + 1.2 * s, start[1] + 0.8 * np.sin(1.5 * s), start[2] + 0.25 * s], axis=1)
    if n_beams is None:
        clean = synth.raycast(poses)
    else:
        clean = synth.raycast(poses, n_beams, synth.ANGLE_MIN, np.float32(4.712389 / float(n_beams - 1)))
    ranges = np.where(clean > 0, clean + rng.normal(0, 0.01, clean.shape), 0.0).astype(np.float32)
    return ranges, np.stack([_rel(poses[0], p) for p in poses])


def _state(m):
    """everything the library shows of a map (takes a pending speculative build back, as any inspection does)"""
    cells = m.cells()
    info = m.info()
    return {
        "cells_int": np.array([[c["index"], c["count"], int(c["built"]), c["slot"]] for c in cells], dtype=np.int64).reshape(-1, 4),
        "cells_mean": np.array([c["mean"] for c in cells]).reshape(-1, 2),
        "cells_icov": np.array([c["icov"] for c in cells]).reshape(-1, 4),
        "points": m.points(),
        "points_slot0": m.points(slot0_only=True),
        "info": np.array([int(info[k]) for k in INFO], dtype=np.int64),
    }


def _assert_same_map(a, b, what):
    sa, sb = _state(a), _state(b)
    for k in sa:
        assert sa[k].shape == sb[k].shape and np.array_equal(sa[k], sb[k]), (what, k, sa[k].shape, sb[k].shape)
    return sa


def _single_update(m, scan, pose, speculate):
    """the single calls an update job stands for"""
    p = np.ascontiguousarray(pose, dtype=np.float64)
    m.mark_unbuilt()
    m._ctx._chk(m._lib.ndtpso_map_insert(m._h, scan._h, p.ctypes.data_as(C.POINTER(C.c_double))))
    if speculate:
        m.speculate_build()


def _assert_same_alignment(a, b, what):
    assert np.array_equal(a[0], b[0]) and a[1] == b[1], (what, a[0], b[0], a[1], b[1])
    for k in ("status", "n_points", "n_built", "gbest_updates"):
        assert int(a[2][k]) == int(b[2][k]), (what, k, a[2][k], b[2][k])


class _Twins:
    """n maps twice (set 0: the batch entries, set 1: the single calls), a resident scan per map and set"""

    def __init__(self, ctx, grids, og=None, pool_bytes=16 << 20, capacity=4096):
        from ndtpso_slam_amd import capi
        self.ctx, self.grids = ctx, grids
        og = og or [0.0] * len(grids)
        self.maps = [[capi.ResidentMap(ctx, g, og_cell_size=o, pool_bytes=pool_bytes) for g, o in zip(grids, og)] for _ in range(2)]
        self.scans = [[capi.ResidentScan(ctx, capacity) for _ in grids] for _ in range(2)]

    def load(self, ranges, geom, clip=True, which=None):
        """ranges[i] into scan i of both sets: one ndtpso_points_load_scans for set 0, load_scan calls for set 1"""
        from ndtpso_slam_amd import capi
        which = range(len(self.grids)) if which is None else which
        rc = capi.load_scans(self.ctx, [(self.scans[0][i], ranges[i], geom, None, self.grids[i] if clip else None, False) for i in which])
        assert (rc == 0).all(), rc
        for i in which:
            self.scans[1][i].load_scan(ranges[i], geom, clip=self.grids[i] if clip else None)

    def update(self, poses, speculate, which=None):
        from ndtpso_slam_amd import capi
        which = list(range(len(self.grids)) if which is None else which)
        rc, route = capi.update_maps(self.ctx, [(self.maps[0][i], self.scans[0][i], poses[i], speculate[i]) for i in which])
        assert (rc == 0).all(), rc
        for i in which:
            _single_update(self.maps[1][i], self.scans[1][i], poses[i], speculate[i])
        return route

    def same(self, what):
        for i in range(len(self.grids)):
            _assert_same_map(self.maps[0][i], self.maps[1][i], (what, i))
            assert np.array_equal(self.scans[0][i].get(), self.scans[1][i].get()), (what, i)

    def close(self):
        for objs in (self.maps, self.scans):
            for row in objs:
                for o in row:
                    o.close()


def test_different_maps_in_one_call(ctx):
    """Five maps -- 60 m at 0.5 m, 60 m at 0.25 m, 40 m at 1 m, a W != H grid, one with an occupancy grid --, eight steps, the
    speculation flag on three of them, an alignment batch between the steps (behind speculative builds nothing has inspected:
    late window binding on both twins)."""
    from ndtpso_slam_amd import capi
    grids = [capi.Grid(60, 60, 0.5), capi.Grid(60, 60, 0.25), capi.Grid(40, 40, 1.0), capi.Grid(40, 20, 0.5), capi.Grid(60, 60, 0.5)]
    starts = [(2.0, -1.0, 0.3), (-6.0, 3.0, -0.8), (4.0, 4.0, 2.0), (-3.0, -5.0, 1.1), (1.0, 2.0, -2.0)]
    speculate = [True, False, True, False, True]
    t = _Twins(ctx, grids, og=[0.0, 0.0, 0.0, 0.0, 0.25], pool_bytes=32 << 20)
    geom, cfg = _geom(), capi.PSOConfig.make(50, 30)
    traj = [_trajectory(10, s, 20 + i) for i, s in enumerate(starts)]
    n = len(grids)
    try:
        for k in range(8):
            t.load([traj[i][0][k] for i in range(n)], geom)
            if k > 0:
                res = [capi.align_maps(ctx, [(t.maps[s][i], t.scans[s][i], traj[i][1][k - 1], DEV, 100 + 10 * k + i) for i in range(n)],
                                       cfg, capi.SCORE_EXACT) for s in range(2)]
                assert (res[0][3] == 0).all() and (res[1][3] == 0).all(), (k, res[0][3], res[1][3])
                assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1]), k
                for key in ("status", "n_points", "n_built", "gbest_updates"):
                    assert np.array_equal(res[0][2][key], res[1][2][key]), (k, key)
            route = t.update([traj[i][1][k] for i in range(n)], speculate)
            if k >= 1:
                assert (route == 1).all(), (k, route)        # pools sized, undo logs and pinned headers allocated: shared launches
            if k in (0, 3):
                t.same(("step", k))
        # after the last step: the alignments of a ninth scan, fp64 score and exact mode, single calls on both twins
        t.load([traj[i][0][8] for i in range(n)], geom)
        for mode in (capi.SCORE_F64, capi.SCORE_EXACT):
            for i in range(n):
                a = t.maps[0][i].align(t.scans[0][i], traj[i][1][7], DEV, cfg, seed=7 + i, mode=mode)
                b = t.maps[1][i].align(t.scans[1][i], traj[i][1][7], DEV, cfg, seed=7 + i, mode=mode)
                _assert_same_alignment(a, b, (mode, i))
        t.same("end")
        og0, og1 = t.maps[0][4].occupancy(), t.maps[1][4].occupancy()
        assert np.array_equal(og0[0], og1[0]) and og0[1:] == og1[1:]
    finally:
        t.close()


def test_loads_of_mixed_geometries_transforms_and_appends(ctx):
    """1081- and 361-beam scans in one call, with and without transform and clip, an append job, the same scan buffer twice (order
    kept), a scan without a valid beam beside full ones."""
    from ndtpso_slam_amd import capi
    g1081, g361 = _geom(), _geom(361)
    r1081, _ = _trajectory(4, (2.0, -1.0, 0.3), 5)
    r361, _ = _trajectory(3, (-4.0, 2.0, 1.0), 6, n_beams=361)
    clip = capi.Grid(40, 20, 40.0)
    sets = [[capi.ResidentScan(ctx, 4096) for _ in range(5)] for _ in range(2)]
    try:
        for s in sets:                                   # scan 3 holds a scan already: the append job adds to it
            s[3].load_scan(r1081[3], g1081, clip=clip)

        def jobs(s):
            return [(s[0], r1081[0], g1081, None, None, False),
                    (s[1], r361[0], g361, (0.4, -0.2, 0.3), clip, False),
                    (s[2], r1081[1], g1081, (-1.0, 2.0, -0.7), None, False),
                    (s[3], r361[1], g361, None, clip, True),
                    (s[4], np.zeros(1081, dtype=np.float32), g1081, None, clip, False),
                    (s[0], r1081[2], g1081, (0.1, 0.1, 0.05), clip, True),      # scan 0 again: behind its first load
                    (s[4], r361[2], g361, None, None, True)]                     # ... and onto the empty one
        rc = capi.load_scans(ctx, jobs(sets[0]))
        assert (rc == 0).all(), rc
        for scan, ranges, geom, trans, cl, append in jobs(sets[1]):
            scan.load_scan(ranges, geom, trans=trans, clip=cl, append=append)
        got = [s.get() for s in sets[0]]
        want = [s.get() for s in sets[1]]
        for i, (a, b) in enumerate(zip(got, want)):
            assert a.shape == b.shape and np.array_equal(a, b), (i, a.shape, b.shape)
        assert got[0].shape[0] > 1081 and got[3].shape[0] > 1081 and 0 < got[4].shape[0] <= 361, [g.shape for g in got]
        # a scan that does not fit is its job's error, the other jobs are completed
        small = [capi.ResidentScan(ctx, 512) for _ in range(2)]
        rc = capi.load_scans(ctx, [(sets[0][1], r361[2], g361, None, None, False), (small[0], r1081[0], g1081, None, None, False),
                                   (sets[0][2], r361[0], g361, None, clip, False)])
        assert list(rc) == [0, capi.E_CAPACITY, 0], rc
        sets[1][1].load_scan(r361[2], g361)
        sets[1][2].load_scan(r361[0], g361, clip=clip)
        for i in (1, 2):
            assert np.array_equal(sets[0][i].get(), sets[1][i].get()), i
        for s in small:
            s.close()
    finally:
        for s in sets:
            for scan in s:
                scan.close()


def test_tile_loop_beside_single_tile_jobs(ctx):
    """A point list of 2162 points (two appended 1081-beam loads: more than the insert's 2048-point tile) as one update job beside
    single-tile jobs."""
    from ndtpso_slam_amd import capi
    grids = [capi.Grid(40, 40, 0.5)] * 3
    t = _Twins(ctx, grids)
    geom = _geom()
    ranges, poses = _trajectory(6, (2.0, -1.0, 0.3), 31)
    try:
        for k in range(2):
            t.load([ranges[3 * k + i] for i in range(3)], geom)
            for s in range(2):                           # scan 1 of both sets gets a second scan appended
                t.scans[s][1].load_scan(ranges[(3 * k + 4) % 6], geom, trans=(0.05, 0.0, 0.01), clip=grids[1], append=True)
            assert t.scans[0][1].get().shape[0] > 2048
            route = t.update([poses[3 * k + i] for i in range(3)], [True, True, False])
            if k == 1:
                assert (route == 1).all(), route
            t.same(("call", k))
    finally:
        t.close()


def test_window_rotation_and_wrap(ctx):
    """One 1 m-cell map and one 0.5 m map updated 105 times with the same scan, taken 0.6 m from a wall: the cells there get more
    than 50 points per build, rotate at every build, wrap the window's 100 slots and give chunks back to the pool."""
    from ndtpso_slam_amd import capi, synth
    grids = [capi.Grid(40, 40, 1.0), capi.Grid(40, 40, 0.5)]
    t = _Twins(ctx, grids, pool_bytes=64 << 20)
    geom = _geom()
    scan = synth.raycast(np.array([[6.0, -4.4, -np.pi / 2]]))[0].astype(np.float32)
    zero = np.zeros(3)
    try:
        t.load([scan, scan], geom)
        for step in range(1, 106):
            route = t.update([zero, zero], [True, True])
            if step > 1:
                assert (route == 1).all(), (step, route)
            for s in range(2):                           # the build an alignment would ask for: commits the speculative one
                for m in t.maps[s]:
                    m.build()
            if step in (1, 51, 101, 105):
                for i in range(2):
                    st = _assert_same_map(t.maps[0][i], t.maps[1][i], (step, i))
                    slots = st["cells_int"][:, 3]        # a cell that rotates at every build is in slot `step` of 100
                    assert (step % 100) in slots and (step > 99 or slots.max() == step), (step, i, slots.max())
    finally:
        t.close()


def test_ordering_and_fallbacks(ctx):
    """The same map twice in one call; a map that is built when the call comes; two update calls with no alignment between them
    (the first speculation is taken back); empty scans with the speculation flag; a call of one job."""
    from ndtpso_slam_amd import capi
    grids = [capi.Grid(40, 40, 0.5)] * 3
    t = _Twins(ctx, grids)
    geom, cfg = _geom(), capi.PSOConfig.make(20, 20)
    ranges, poses = _trajectory(9, (2.0, -1.0, 0.3), 41)
    try:
        t.load([ranges[i] for i in range(3)], geom)
        t.update([poses[i] for i in range(3)], [True, True, True])           # first call: allocations, any route
        # two calls in a row: the speculative builds of the first are taken back by the second's inserts
        t.load([ranges[3 + i] for i in range(3)], geom)
        route = t.update([poses[3 + i] for i in range(3)], [True, True, True])
        assert (route == 1).all(), route
        # the same map twice in one call, with two different scans, beside another map: per map, job order
        jobs = lambda s: [(t.maps[s][0], t.scans[s][0], poses[4], True), (t.maps[s][1], t.scans[s][1], poses[5], True),  # noqa: E731
                          (t.maps[s][0], t.scans[s][2], poses[6], True)]
        rc, route = capi.update_maps(ctx, jobs(0))
        assert (rc == 0).all() and (route == 1).all(), (rc, route)
        for m, scan, pose, spec in jobs(1):
            _single_update(m, scan, pose, spec)
        # alignments behind those speculative builds, then a map that is built when the call comes
        for i in range(2):
            a = t.maps[0][i].align(t.scans[0][i], poses[6], DEV, cfg, seed=3, mode=capi.SCORE_EXACT)
            b = t.maps[1][i].align(t.scans[1][i], poses[6], DEV, cfg, seed=3, mode=capi.SCORE_EXACT)
            _assert_same_alignment(a, b, ("after repeats", i))
        for s in range(2):
            t.maps[s][2].build()
        t.load([ranges[6 + i] for i in range(3)], geom)
        t.update([poses[6 + i] for i in range(3)], [True, False, True])
        t.same("built maps")
        # empty scans and the speculation flag: a buffer never loaded (no points by the host's own bound) and a scan without a
        # valid beam (none on the device) -- nothing is inserted, the flagged build is still made
        empty = [capi.ResidentScan(ctx, 2048) for _ in range(2)]
        blank = np.zeros(1081, dtype=np.float32)
        t.load([blank, blank, blank], geom, which=[1])
        rc, route = capi.update_maps(ctx, [(t.maps[0][0], empty[0], poses[0], True), (t.maps[0][1], t.scans[0][1], poses[1], True),
                                           (t.maps[0][2], t.scans[0][2], poses[2], False)])
        assert (rc == 0).all() and (route == 1).all(), (rc, route)
        _single_update(t.maps[1][0], empty[1], poses[0], True)
        _single_update(t.maps[1][1], t.scans[1][1], poses[1], True)
        _single_update(t.maps[1][2], t.scans[1][2], poses[2], False)
        for i in range(3):
            a = t.maps[0][i].align(t.scans[0][2], poses[8], DEV, cfg, seed=5, mode=capi.SCORE_F64)
            b = t.maps[1][i].align(t.scans[1][2], poses[8], DEV, cfg, seed=5, mode=capi.SCORE_F64)
            _assert_same_alignment(a, b, ("after empty scans", i))
        t.same("empty scans")
        # a call of one job is the single calls
        rc, route = capi.update_maps(ctx, [(t.maps[0][0], t.scans[0][0], poses[3], True)])
        assert list(rc) == [0] and list(route) == [0], (rc, route)
        _single_update(t.maps[1][0], t.scans[1][0], poses[3], True)
        t.same("one job")
        for e in empty:
            e.close()
    finally:
        t.close()


def test_pool_that_must_grow_mid_sequence(ctx):
    """Pools of 64 chunks: the host's bound reaches them at once, the jobs that must measure or grow their pool take the single
    calls in their place in job order (route 0), the others the shared launches, and the maps are the single calls' throughout."""
    from ndtpso_slam_amd import capi
    grids = [capi.Grid(40, 40, 0.5)] * 3
    t = _Twins(ctx, grids, pool_bytes=64 * 512)
    geom = _geom()
    ranges, poses = _trajectory(8, (2.0, -1.0, 0.3), 51)
    seen = set()
    try:
        for k in range(8):
            t.load([ranges[(k + i) % 8] for i in range(3)], geom)
            route = t.update([poses[(k + i) % 8] for i in range(3)], [True, k % 2 == 0, False])
            seen.update(int(r) for r in route)
            if k in (0, 3, 7):
                t.same(("step", k))
        assert seen == {0, 1}, seen
        assert all(m.info()["status"] == 0 for m in t.maps[0])      # grown, never exhausted
    finally:
        t.close()


def test_a_map_of_another_context_is_refused_before_anything_is_enqueued(ctx):
    from ndtpso_slam_amd import capi
    grid = capi.Grid(40, 40, 0.5)
    t = _Twins(ctx, [grid, grid])
    other = capi.Context(0)
    foreign_map = capi.ResidentMap(other, grid, pool_bytes=16 << 20)
    foreign_scan = capi.ResidentScan(other, 2048)
    geom = _geom()
    ranges, poses = _trajectory(4, (2.0, -1.0, 0.3), 61)
    try:
        t.load([ranges[0], ranges[1]], geom)
        t.update([poses[0], poses[1]], [True, True])
        t.load([ranges[2], ranges[3]], geom)
        for bad in ([(t.maps[0][0], t.scans[0][0], poses[2], True), (foreign_map, t.scans[0][1], poses[3], True)],
                    [(t.maps[0][0], t.scans[0][0], poses[2], True), (t.maps[0][1], foreign_scan, poses[3], True)]):
            with pytest.raises(capi.NdtpsoError) as e:
                capi.update_maps(ctx, bad)
            assert e.value.code == capi.E_ARG
        with pytest.raises(capi.NdtpsoError) as e:
            capi.load_scans(ctx, [(t.scans[0][0], ranges[0], geom, None, grid, False), (foreign_scan, ranges[1], geom, None, grid, False)])
        assert e.value.code == capi.E_ARG
        t.same("nothing was enqueued")                        # set 1 was not touched since the loads either
    finally:
        foreign_map.close()
        foreign_scan.close()
        other.close()
        t.close()
