"""ndtpso_map_search_batch / capi.search_maps: several lattice searches of one context in shared launches.

The contract (include/ndtpso_hip.h) is the single call's: per job, poses, costs, indices and every field of the stats are bit
for bit what ResidentMap.search returns for the same arguments, in all three score modes.  The reference of every test here is
therefore ResidentMap.search, job by job, compared with tobytes() / ==."""
import ctypes as C

import numpy as np
import pytest

import search_case as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def case(ctx):
    return sc.device_case(ctx)


@pytest.fixture(scope="module")
def case_30cm(ctx):
    return sc.device_case(ctx, cell_side=0.3)


def _modes():
    from ndtpso_slam_amd import capi
    return (capi.SCORE_F64, capi.SCORE_EXACT, capi.SCORE_F32)


def _same(got, want, what=""):
    """a job's result against ResidentMap.search's tuple"""
    for g, w in zip(got[:3], want[:3]):
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), (what, g, w)
    assert got[3] == want[3], (what, got[3], want[3])


def _check(ctx, jobs, mode, what="", route=1):
    """the batch against the single calls, job by job; returns (results, batch stats)"""
    from ndtpso_slam_amd import capi
    want = [m.search(s, origin, step, count, top_k, mode=mode) for m, s, origin, step, count, top_k in jobs]
    got, bs = capi.search_maps(ctx, jobs, mode=mode)
    assert len(got) == len(jobs)
    for j, (g, w) in enumerate(zip(got, want)):
        assert g[4] == capi.OK and g[5] == route, (what, mode, j, g[4:])
        _same(g, w, (what, mode, j))
    return got, bs


def _few_points(ctx, s, n):
    from ndtpso_slam_amd import capi
    few = capi.ResidentScan(ctx, sc.N_BEAMS)
    few.set(s.get()[:n])
    return few


def test_mixed_batch(ctx, case, case_30cm):
    """three maps, three scans of 361, 65 and 1 points, three lattices and three top_k; the lattice of one node lies between the
    others, so a job of one node sits between part boundaries"""
    from ndtpso_slam_amd import capi
    m0, s0 = case
    m1, s1 = case_30cm
    m2, s2 = sc.device_case(ctx, poses=sc.MAP_POSES[:4])
    jobs = [(m0, s0, sc.ORIGIN, sc.STEP, (9, 9, 16), 8),
            (m1, _few_points(ctx, s1, 1), (0.9, -1.3, 0.3), sc.STEP, (1, 1, 1), 1),
            (m2, _few_points(ctx, s2, 65), (0.9, -1.3, 0.3), sc.STEP, (17, 3, 2), 64)]
    for mode in _modes():
        got, bs = _check(ctx, jobs, mode, "mixed")
        assert bs["single_jobs"] == 0 and bs["launches"] > 0 and bs["waits"] > 0, bs
        assert [g[3]["n_points"] for g in got] == [len(s0.get()), 1, 65]
    exact = capi.search_maps(ctx, jobs, mode=capi.SCORE_EXACT)[0]
    assert exact[0][3]["mode_run"] == capi.SCORE_F32 and exact[0][3]["fell_back"] == 0 and exact[0][3]["path"] == 2, exact[0][3]


def test_one_scan_many_maps(ctx, case, case_30cm):
    """which submap is this scan from: one scan against three maps, one of them built only far from the lattice, so that all its
    costs are 0 and its exact mode sweeps in fp64 -- alone: the others keep the fp32 sweep"""
    from ndtpso_slam_amd import capi
    m0, s = case
    m1, _ = case_30cm
    far = capi.ResidentMap(ctx, capi.Grid(sc.FRAME_M, sc.FRAME_M, sc.CELL_SIDE), pool_bytes=64 << 20)
    far.insert_host(np.array([-25.0, -25.0]) + 0.05 + np.array([[0.01, 0.02], [0.05, 0.07], [0.1, 0.03], [0.12, 0.11]]), (0, 0, 0))
    far.build()
    jobs = [(m, s, sc.ORIGIN, sc.STEP, (9, 9, 4), 8) for m in (m0, far, m1)]
    for mode in _modes():
        got, _ = _check(ctx, jobs, mode, "one scan")
        if mode == capi.SCORE_EXACT:
            assert got[1][3]["fell_back"] == capi.SEARCH_FELL_UNDERFLOW and got[1][3]["mode_run"] == capi.SCORE_F64, got[1][3]
            for j in (0, 2):
                assert got[j][3]["mode_run"] == capi.SCORE_F32 and got[j][3]["fell_back"] == 0, got[j][3]
        assert (got[1][1] == 0).all() and got[1][2].tolist() == list(range(8))


def test_one_map_several_lattices(ctx, case):
    """(33, 32, 5) = 5280 nodes: the first selection stage of that job has two parts"""
    m, s = case
    jobs = [(m, s, sc.ORIGIN, sc.STEP, (5, 4, 3), 8),
            (m, s, (-1.0, -3.0, 0.2), (0.1, 0.1, 0.1), (33, 32, 5), 16),
            (m, s, (0.9, -1.3, 0.3), sc.STEP, (7, 1, 1), 64)]
    for mode in _modes():
        got, _ = _check(ctx, jobs, mode, "lattices")
        assert got[1][3]["n_nodes"] == 5280 and len(got[2][2]) == 7


def test_mixed_kinds(ctx, case):
    """the 300 m / 0.25 m map of test_every_table_plan (bitmap in LDS: path 1, the exact mode falls back by plan) beside the
    verified case (dense, path 2) in one call: two kernel kinds"""
    from ndtpso_slam_amd import capi
    cell_side, reach = 0.25, 50.0
    grid = capi.Grid(300, 300, cell_side)
    big = capi.ResidentMap(ctx, grid)
    sb = capi.ResidentScan(ctx, sc.N_BEAMS)
    maps, query = sc.ranges()
    sb.load_scan(maps[2], sc.geom(), clip=grid)
    big.insert(sb, (0, 0, 0))
    sb.load_scan(query, sc.geom(), clip=grid)
    inside = 0.05 + np.array([[0.01, 0.02], [0.05, 0.07], [0.1, 0.03], [0.12, 0.11]])
    lo, hi = int((150.0 - reach) / cell_side), int((150.0 + reach) / cell_side)
    big.insert_host(np.concatenate([lo * cell_side - 150.0 + inside, hi * cell_side - 150.0 + inside]), (0, 0, 0))
    big.build()
    m, s = case
    jobs = [(big, sb, (1.0, -1.0, 0.4), (0.2, 0.2, 0.05), (5, 3, 2), 8), (m, s, sc.ORIGIN, sc.STEP, sc.COUNT, sc.TOP_K)]
    for mode in _modes():
        got, bs = _check(ctx, jobs, mode, "kinds")
        assert got[0][3]["path"] == 1, got[0][3]
        if mode == capi.SCORE_EXACT:
            assert got[0][3]["fell_back"] == capi.SEARCH_FELL_PLAN and got[0][3]["mode_run"] == capi.SCORE_F64, got[0][3]
            assert got[1][3]["path"] == 2 and got[1][3]["fell_back"] == 0, got[1][3]


def test_equal_costs(ctx, case):
    """headings 2 pi apart as one job among others: equal costs are ordered by index, whatever the dealing"""
    m, s = case
    jobs = [(m, s, sc.ORIGIN, sc.STEP, (3, 3, 2), 4),
            (m, s, (0.9, -1.3, -np.pi), (0.3, 0.3, 2 * np.pi), (5, 4, 2), 16),
            (m, s, sc.ORIGIN, sc.STEP, (9, 9, 4), 8)]
    for mode in _modes():
        _check(ctx, jobs, mode, "two pi")


def test_map_state(ctx):
    """one job's map has an unbuilt insert, another's a pending speculation: hits as the single calls', and every map left as the
    single call leaves an identically prepared one"""
    from ndtpso_slam_amd import capi

    def prepared(pending):
        m, s = sc.device_case(ctx, poses=sc.MAP_POSES[:4], build=False)
        if pending == "speculation":
            m.build()
            maps, query = sc.ranges()
            s.load_scan(maps[4], sc.geom(), clip=m.grid)
            m.insert(s, np.asarray(sc.MAP_POSES[4]))
            m.speculate_build()
            s.load_scan(query, sc.geom(), clip=m.grid)
        return m, s

    lattice = (sc.ORIGIN, sc.STEP, (9, 9, 4), 8)
    for mode in (capi.SCORE_EXACT, capi.SCORE_F64):
        batch = [prepared("insert"), prepared("speculation")]
        alone = [prepared("insert"), prepared("speculation")]
        got, _ = capi.search_maps(ctx, [(m, s) + lattice for m, s in batch], mode=mode)
        for (m, s), (mb, _), g in zip(alone, batch, got):
            want = m.search(s, *lattice, mode=mode)
            assert g[4] == capi.OK and g[5] == 1
            _same(g, want, ("state", mode))
            assert mb.info() == m.info()


@pytest.mark.parametrize("mode_name", ["F64", "EXACT"])
def test_launch_counts(ctx, case, mode_name):
    """jobs of one kernel kind: the launches and the waits for the stream do not depend on the number of jobs"""
    from ndtpso_slam_amd import capi
    mode = getattr(capi, "SCORE_" + mode_name)
    m, s = case
    job = (m, s, sc.ORIGIN, sc.STEP, sc.COUNT, sc.TOP_K)
    _, two = _check(ctx, [job] * 2, mode, "2 jobs")
    _, eight = _check(ctx, [job] * 8, mode, "8 jobs")
    assert two["launches"] == eight["launches"] and two["waits"] == eight["waits"], (two, eight)
    assert two["single_jobs"] == eight["single_jobs"] == 0
    # a single call in F64 is a sweep and two selection launches (search_sweep); the exact mode adds a collect and a cost launch
    assert eight["launches"] < 8 * 3, eight
    if mode == capi.SCORE_F64:
        assert eight["launches"] == 3, eight


def _job_array(jobs):
    from ndtpso_slam_amd import capi
    arr = (capi.MapSearchJob * len(jobs))()
    keep = []
    for j, (m, s, origin, step, count, top_k) in zip(arr, jobs):
        j.map, j.new_points = m._h, s._h
        j.lattice = capi.Lattice((C.c_double * 3)(*origin), (C.c_double * 3)(*step), (C.c_uint32 * 3)(*count), top_k)
        hits = (capi.LatticeHit * 64)()
        keep.append(hits)
        j.hits = hits
        j.rc, j.route, j.n_hits = 77, 77, 77
    return arr, keep


def test_errors(ctx, case):
    from ndtpso_slam_amd import capi
    m, s = case
    L = ctx._lib
    good = (m, s, sc.ORIGIN, sc.STEP, (3, 3, 2), 4)

    def untouched(arr):
        return all(j.rc == 77 and j.route == 77 and j.n_hits == 77 for j in arr)

    arr, keep = _job_array([good, good])
    f64 = capi.SCORE_F64
    assert L.ndtpso_map_search_batch(None, arr, 2, f64, None) == capi.E_ARG
    assert L.ndtpso_map_search_batch(ctx._h, None, 2, f64, None) == capi.E_ARG
    assert L.ndtpso_map_search_batch(ctx._h, arr, 0, f64, None) == capi.E_ARG
    assert L.ndtpso_map_search_batch(ctx._h, arr, 2, 7, None) == capi.E_ARG
    for field in ("map", "new_points", "hits"):
        bad, keep_bad = _job_array([good, good])
        setattr(bad[1], field, None)
        assert L.ndtpso_map_search_batch(ctx._h, bad, 2, f64, None) == capi.E_ARG, field
        assert untouched(bad), field
    other = capi.Context(0)
    try:
        foreign = capi.ResidentScan(other, sc.N_BEAMS)
        foreign.set(s.get())
        bad, keep_bad = _job_array([good, (m, foreign) + good[2:]])
        assert L.ndtpso_map_search_batch(ctx._h, bad, 2, f64, None) == capi.E_ARG
        assert untouched(bad)
        foreign.close()
    finally:
        other.close()
    assert untouched(arr)
    # two lattices of 2^24 nodes each: valid alone, together more than the shared cost buffer holds
    huge, keep_huge = _job_array([(m, s, sc.ORIGIN, sc.STEP, (4096, 4096, 1), 4)] * 2)
    assert L.ndtpso_map_search_batch(ctx._h, huge, 2, f64, None) == capi.E_ARG
    assert untouched(huge)
    # ... and a following good call works (stats may be NULL)
    assert L.ndtpso_map_search_batch(ctx._h, arr, 2, f64, None) == capi.OK
    assert all(j.rc == capi.OK and j.route == 1 and j.n_hits == 4 for j in arr)
    _check(ctx, [good, good], f64, "after the errors")

    # a middle job whose own lattice the single call refuses: its rc, the call's return, and the others complete
    jobs = [good, (m, s, sc.ORIGIN, sc.STEP, (0, 3, 2), 4), (m, s, sc.ORIGIN, sc.STEP, (9, 9, 4), 8)]
    for mode in _modes():
        arr3, keep3 = _job_array(jobs)
        bs = capi.SearchBatchStats()
        assert L.ndtpso_map_search_batch(ctx._h, arr3, 3, mode, C.byref(bs)) == capi.E_ARG
        assert arr3[1].rc == capi.E_ARG and arr3[1].n_hits == 0
        for j in (0, 2):
            want = m.search(s, *jobs[j][2:], mode=mode)
            assert arr3[j].rc == capi.OK and arr3[j].route == 1
            _same(capi._search_result(keep3[j], arr3[j].n_hits, arr3[j].stats), want, ("middle", mode, j))
    got, bs = capi.search_maps(ctx, jobs, mode=capi.SCORE_EXACT)
    assert [g[4] for g in got] == [capi.OK, capi.E_ARG, capi.OK] and len(got[1][2]) == 0

    # two jobs of which one is refused: the other is the only one left, and runs as the single call (route 0, no shared launch)
    arr2, keep2 = _job_array([jobs[1], jobs[2]])
    bs = capi.SearchBatchStats()
    assert L.ndtpso_map_search_batch(ctx._h, arr2, 2, capi.SCORE_EXACT, C.byref(bs)) == capi.E_ARG
    assert arr2[0].rc == capi.E_ARG and arr2[0].n_hits == 0 and arr2[1].rc == capi.OK and arr2[1].route == 0
    _same(capi._search_result(keep2[1], arr2[1].n_hits, arr2[1].stats), m.search(s, *jobs[2][2:], mode=capi.SCORE_EXACT), "one left")
    assert bs.launches == 0 and bs.single_jobs == 1, (bs.launches, bs.waits, bs.single_jobs)

    # one job alone is the single call
    got, bs = _check(ctx, [good], capi.SCORE_EXACT, "alone", route=0)
    assert bs == {"launches": 0, "waits": 0, "single_jobs": 1}, bs
