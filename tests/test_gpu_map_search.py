"""ndtpso_map_search / ResidentMap.search: cost_function at every node of a pose lattice against a resident map, the best
top_k nodes picked on the device.

The contract (include/ndtpso_hip.h): in SCORE_F64 the hits are exactly the best of ResidentMap.cost(F64) over
capi.lattice_poses, in stable-argsort order, costs and poses bit for bit; SCORE_EXACT returns the same bits from the fp32
sweep wherever its margin is proven and says why where it is not; SCORE_F32 is a tolerance mode.  The reference of every
test here is therefore the brute force a caller had to write before -- every pose through ResidentMap.cost, sorted on the
host -- and, for the verified case, the CPU oracle."""
import ctypes as C

import numpy as np
import pytest

import search_case as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def case(ctx):
    return sc.device_case(ctx)


@pytest.fixture(scope="module")
def case_brute(case):
    """the brute force over the verified case's lattice, computed once"""
    from ndtpso_slam_amd import capi
    m, s = case
    poses, costs, order = sc.brute(m, s, sc.ORIGIN, sc.STEP, sc.COUNT, sc.TOP_K, capi)
    costs.setflags(write=False)
    return poses, costs, order


def _assert_is_brute(got, poses, costs, order, what=""):
    g_poses, g_costs, g_index, _ = got
    assert g_index.tolist() == order.tolist(), (what, g_index, order)
    assert g_costs.tobytes() == costs[order].tobytes(), (what, g_costs, costs[order])
    assert g_poses.tobytes() == poses[order].tobytes(), (what, g_poses, poses[order])


def _check_against_brute(m, s, origin, step, count, top_k, what="", modes=None):
    from ndtpso_slam_amd import capi
    poses, costs, order = sc.brute(m, s, origin, step, count, top_k, capi)
    stats = {}
    for mode in modes or (capi.SCORE_F64, capi.SCORE_EXACT):
        got = m.search(s, origin, step, count, top_k, mode=mode)
        _assert_is_brute(got, poses, costs, order, (what, mode))
        st = got[3]
        assert st["n_nodes"] == len(costs) and st["n_points"] == len(s.get()), (what, st)
        if mode == capi.SCORE_F64:
            assert st["mode_run"] == capi.SCORE_F64 and st["fell_back"] == 0 and st["n_candidates"] == 0, (what, st)
        else:
            # the fp32 sweep and its candidates, or the fp64 sweep and a reason
            assert (st["mode_run"] == capi.SCORE_F32 and st["fell_back"] == 0 and
                    min(top_k, len(costs)) <= st["n_candidates"] <= capi.SEARCH_MAX_CANDIDATES) or \
                   (st["mode_run"] == capi.SCORE_F64 and st["fell_back"] != 0 and st["n_candidates"] == 0), (what, st)
        stats[mode] = st
    return stats


def test_verified_case(case, case_brute):
    from ndtpso_slam_amd import capi
    m, s = case
    poses, costs, order = case_brute
    n = len(s.get())
    tau = sc.TAU_PER_POINT * n
    assert np.array_equal(poses, capi.lattice_poses(sc.ORIGIN, sc.STEP, sc.COUNT))

    f64 = m.search(s, sc.ORIGIN, sc.STEP, sc.COUNT, sc.TOP_K, mode=capi.SCORE_F64)
    _assert_is_brute(f64, poses, costs, order, "F64")
    assert f64[3]["mode_run"] == capi.SCORE_F64 and f64[3]["path"] == 1 and f64[3]["n_nodes"] == 9 * 9 * 16

    # the oracle: same nodes in the same order, costs to the suite's tolerance for device costs
    _, _, o_costs = sc.oracle_case()
    o_order = np.argsort(o_costs, kind="stable")
    gaps = np.diff(o_costs[o_order[:sc.TOP_K + 1]])
    assert gaps.min() > 1e-6, gaps              # (the oracle alone: 5.2e-3, so the order is not a matter of rounding)
    assert int(o_order[0]) == 688
    assert f64[2].tolist() == o_order[:sc.TOP_K].tolist()
    np.testing.assert_allclose(f64[1], o_costs[o_order[:sc.TOP_K]], rtol=1e-9, atol=0)

    exact = m.search(s, sc.ORIGIN, sc.STEP, sc.COUNT, sc.TOP_K, mode=capi.SCORE_EXACT)
    _assert_is_brute(exact, poses, costs, order, "EXACT")
    st = exact[3]
    assert st["mode_run"] == capi.SCORE_F32 and st["path"] == 2 and st["fell_back"] == 0, st
    assert 8 <= st["n_candidates"] <= 4096, st

    f32 = m.search(s, sc.ORIGIN, sc.STEP, sc.COUNT, sc.TOP_K, mode=capi.SCORE_F32)
    assert f32[3]["mode_run"] == capi.SCORE_F32 and len(f32[2]) == sc.TOP_K
    assert np.array_equal(f32[0], poses[f32[2]])
    assert (np.abs(f32[1] - costs[f32[2]]) <= tau).all(), (f32[1], costs[f32[2]], tau)
    ninth = np.sort(costs, kind="stable")[sc.TOP_K]
    for idx in order:
        assert idx in f32[2] or abs(costs[idx] - ninth) <= tau, (idx, costs[idx], ninth)


@pytest.mark.parametrize("n_points", [1, 63, 64, 65, 361])
def test_point_counts(ctx, case, n_points):
    from ndtpso_slam_amd import capi
    m, s = case
    pts = s.get()
    assert len(pts) >= 361 or n_points < 361
    few = capi.ResidentScan(ctx, sc.N_BEAMS)
    few.set(pts[:n_points])
    _check_against_brute(m, few, sc.ORIGIN, sc.STEP, (5, 4, 3), 8, "n_points %d" % n_points)


@pytest.mark.parametrize("count", [(1, 1, 1), (7, 1, 1), (1, 5, 3), (17, 3, 2)])
@pytest.mark.parametrize("top_k", [1, 64, 200])
def test_counts_and_top_k(case, count, top_k):
    """node counts that are no multiple of a wave or workgroup count; top_k 1, 64 and (where the lattice is smaller) more than the
    nodes.  200 stands for "larger than the node count" through min(): the entry itself refuses top_k > 64."""
    m, s = case
    nodes = count[0] * count[1] * count[2]
    k = min(top_k, 64)
    st = _check_against_brute(m, s, (0.9, -1.3, 0.3), sc.STEP, count, k, (count, top_k))
    assert all(v["n_nodes"] == nodes for v in st.values())
    got = m.search(s, (0.9, -1.3, 0.3), sc.STEP, count, k)
    assert len(got[2]) == min(k, nodes)


def test_equal_costs_two_pi_apart(case):
    """two headings 2 pi apart: the costs of a pair are equal wherever sincos returns the same bits for both, and then the lower
    index comes first -- either way the hits are the brute force's"""
    m, s = case
    _check_against_brute(m, s, (0.9, -1.3, -np.pi), (0.3, 0.3, 2 * np.pi), (5, 4, 2), 16, "two pi")


def test_cells_of_30_cm(ctx):
    """the index path of cells that are no power of two"""
    from ndtpso_slam_amd import capi
    m, s = sc.device_case(ctx, cell_side=0.3)
    st = _check_against_brute(m, s, sc.ORIGIN, sc.STEP, (9, 9, 4), 8, "0.3 m cells")
    assert st[capi.SCORE_F64]["path"] == 0, st


@pytest.mark.parametrize("cell_side,pow2", [(0.25, True), (0.3, False)])
def test_every_table_plan(ctx, cell_side, pow2):
    """One map per table plan make_plan can return for a prebuilt table, the plan asserted: the verified case and the 0.3 m
    case run the tables staged in LDS (fp64: bitmap 1 / 0; fp32: dense 2).  Here a 300 m frame whose built box is first
    ~400 cells a side -- no dense table of that size fits LDS, the bitmap does: fp32 on the bitmap, 1 / 0 -- and then spans the
    frame: no form fits, the table is read from its HBM image, 5 / 4 (the map of
    test_resident_frame_of_a_million_cells_built_from_end_to_end)."""
    from ndtpso_slam_amd import capi
    grid = capi.Grid(300, 300, cell_side)
    m = capi.ResidentMap(ctx, grid)
    s = capi.ResidentScan(ctx, sc.N_BEAMS)
    maps, query = sc.ranges()
    s.load_scan(maps[2], sc.geom(), clip=grid)
    m.insert(s, (0, 0, 0))
    s.load_scan(query, sc.geom(), clip=grid)
    # four points 6 - 17 cm inside the low edge of one cell per corner (more than two points: the cell is built)
    inside = 0.05 + np.array([[0.01, 0.02], [0.05, 0.07], [0.1, 0.03], [0.12, 0.11]])
    for reach, lds_path in ((50.0, 1 if pow2 else 0), (140.0, 5 if pow2 else 4)):
        lo, hi = int((150.0 - reach) / cell_side), int((150.0 + reach) / cell_side)
        m.insert_host(np.concatenate([lo * cell_side - 150.0 + inside, hi * cell_side - 150.0 + inside]), (0, 0, 0))
        m.build()
        info = m.info()
        assert info["x1"] - info["x0"] >= hi - lo and info["y1"] - info["y0"] >= hi - lo, (info, lo, hi)
        assert m.info()["status"] == 0
        st = _check_against_brute(m, s, (1.0, -1.0, 0.4), (0.2, 0.2, 0.05), (5, 3, 2), 8, (cell_side, reach))
        assert st[capi.SCORE_F64]["path"] == lds_path, st
        assert st[capi.SCORE_EXACT]["fell_back"] == capi.SEARCH_FELL_PLAN and st[capi.SCORE_EXACT]["path"] == lds_path, st
        f32 = m.search(s, (1.0, -1.0, 0.4), (0.2, 0.2, 0.05), (5, 3, 2), 8, mode=capi.SCORE_F32)
        assert f32[3]["path"] == lds_path and f32[3]["mode_run"] == capi.SCORE_F32, f32[3]
        costs = m.cost(s, f32[0], mode=capi.SCORE_F64)
        assert (np.abs(f32[1] - costs) <= sc.TAU_PER_POINT * f32[3]["n_points"]).all(), (f32[1], costs)


@pytest.mark.parametrize("empty_scan", [False, True])
def test_all_costs_zero(ctx, case, empty_scan):
    """a lattice wholly outside the built cells, or an empty scan: every cost is zero, so the hits are nodes 0 .. K - 1 in order in
    all three modes, and SCORE_EXACT says that it swept in fp64 (c32_K in the underflow regime)"""
    from ndtpso_slam_amd import capi
    m, s = case
    origin = (-29.5, -29.5, 0.0)
    if empty_scan:
        s = capi.ResidentScan(ctx, sc.N_BEAMS)
        s.set(np.zeros((0, 2)))
        origin = sc.ORIGIN
    for mode in (capi.SCORE_F64, capi.SCORE_EXACT, capi.SCORE_F32):
        poses, costs, index, st = m.search(s, origin, (0.1, 0.1, 0.4), (3, 3, 4), 10, mode=mode)
        assert index.tolist() == list(range(10)) and (costs == 0).all(), (mode, index, costs)
        assert np.array_equal(poses, capi.lattice_poses(origin, (0.1, 0.1, 0.4), (3, 3, 4))[:10])
        if mode == capi.SCORE_EXACT:
            assert st["fell_back"] == capi.SEARCH_FELL_UNDERFLOW and st["mode_run"] == capi.SCORE_F64, st
    assert (m.cost(s, capi.lattice_poses(origin, (0.1, 0.1, 0.4), (3, 3, 4)), mode=capi.SCORE_F64) == 0).all()


@pytest.mark.parametrize("pending", ["insert", "speculation"])
def test_map_state_as_after_map_cost(ctx, pending):
    """A map with an unbuilt insert, and one with a pending speculative build: search returns what it returns after an explicit
    build(), and leaves the map as ndtpso_map_cost in the same position does -- info() and a following align are equal."""
    from ndtpso_slam_amd import capi
    cfg = capi.PSOConfig.make(20, 12)

    def prepared():
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
    m_a, s_a = prepared()
    got = m_a.search(s_a, *lattice, mode=capi.SCORE_EXACT)
    m_b, s_b = prepared()
    m_b.cost(s_b, [sc.TRUTH], mode=capi.SCORE_F64)
    m_c, s_c = prepared()
    m_c.build()
    want = m_c.search(s_c, *lattice, mode=capi.SCORE_EXACT)
    for g, w in zip(got[:3], want[:3]):
        assert g.tobytes() == w.tobytes(), (g, w)
    assert got[3] == want[3]
    assert m_a.info() == m_b.info()
    a = m_a.align(s_a, got[0][0], (0.15, 0.15, 0.03), cfg, seed=5, mode=capi.SCORE_EXACT)
    b = m_b.align(s_b, got[0][0], (0.15, 0.15, 0.03), cfg, seed=5, mode=capi.SCORE_EXACT)
    assert np.array_equal(a[0], b[0]) and a[1] == b[1] and a[2] == b[2], (a, b)
    assert m_a.info() == m_b.info()


def test_argument_errors(ctx, case):
    from ndtpso_slam_amd import capi
    m, s = case
    L = ctx._lib
    good = dict(origin=sc.ORIGIN, step=sc.STEP, count=(3, 3, 2), top_k=4)

    def code(mode=capi.SCORE_F64, scan=s, **kw):
        a = dict(good, **kw)
        with pytest.raises(capi.NdtpsoError) as e:
            m.search(scan, a["origin"], a["step"], a["count"], a["top_k"], mode=mode)
        return e.value.code

    inf, nan = float("inf"), float("nan")
    assert code(count=(0, 3, 2)) == capi.E_ARG
    assert code(count=(3, 3, 0)) == capi.E_ARG
    assert code(count=(4096, 4096, 2)) == capi.E_ARG              # 2^25 nodes
    assert code(count=(65536, 65536, 65536)) == capi.E_ARG        # (a product that wraps 32 and 48 bits)
    assert code(top_k=0) == capi.E_ARG
    assert code(top_k=65) == capi.E_ARG
    for bad in (0.0, -0.3, inf, nan):
        assert code(step=(0.3, bad, 0.06)) == capi.E_ARG, bad
    assert code(origin=(0.0, inf, 0.0)) == capi.E_ARG
    assert code(origin=(nan, 0.0, 0.0)) == capi.E_ARG
    assert code(mode=7) == capi.E_ARG
    other = capi.Context(0)
    try:
        foreign = capi.ResidentScan(other, sc.N_BEAMS)
        foreign.set(s.get())
        assert code(scan=foreign) == capi.E_ARG
        foreign.close()
    finally:
        other.close()
    # null pointers, through the C entry itself
    lat = capi.Lattice((C.c_double * 3)(*sc.ORIGIN), (C.c_double * 3)(*sc.STEP), (C.c_uint32 * 3)(3, 3, 2), 4)
    hits = (capi.LatticeHit * 4)()
    n = C.c_uint32()
    assert L.ndtpso_map_search(None, s._h, C.byref(lat), capi.SCORE_F64, hits, C.byref(n), None) == capi.E_ARG
    assert L.ndtpso_map_search(m._h, None, C.byref(lat), capi.SCORE_F64, hits, C.byref(n), None) == capi.E_ARG
    assert L.ndtpso_map_search(m._h, s._h, None, capi.SCORE_F64, hits, C.byref(n), None) == capi.E_ARG
    assert L.ndtpso_map_search(m._h, s._h, C.byref(lat), capi.SCORE_F64, None, C.byref(n), None) == capi.E_ARG
    assert L.ndtpso_map_search(m._h, s._h, C.byref(lat), capi.SCORE_F64, hits, None, None) == capi.E_ARG
    # a step that is not read (an axis of one node) may be anything, stats may be NULL, and the context still works
    assert L.ndtpso_map_search(m._h, s._h, C.byref(lat), capi.SCORE_F64, hits, C.byref(n), None) == capi.OK and n.value == 4
    _check_against_brute(m, s, sc.ORIGIN, (nan, 0.3, -1.0), (1, 3, 1), 3, "after the errors")
