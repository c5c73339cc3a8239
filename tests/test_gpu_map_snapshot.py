"""ndtpso_map_snapshot / ndtpso_map_restore (ResidentMap.snapshot / ResidentMap.restore) and NDTFrame::save / NDTFrame::load: a
resident map saved to a blob and restored, in another context or another process, behaves under every later operation exactly
as the original would have -- bit for bit.

The map is the one of tests/search_case.py unless a test says otherwise: six scans of 361 beams in a 60 m frame of 0.5 m cells,
with an occupancy grid of 0.1 m where a test looks at it.  The reference of every comparison is the original map itself (the
contract is "the same bits"); where the state matters as such -- the window ring that has wrapped, the pinned blob's cells -- the
CPU oracle is the third party."""
import ctypes as C
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import search_case as sc
import snapshot_case as snc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "host", "replay", "snapshot_check")
POOL = 64 << 20
OG_CELL = 0.1
DEVIATION = (0.1, 0.1, 3.1415e-3)
GUESS = (1.25, -0.65, 0.44)
ENV_OFF = ("NDTPSO_SCORE", "NDTPSO_RESIDENT", "NDTPSO_ALIGN_FRAME_CONFIG", "NDTPSO_SPECULATE", "NDTPSO_LATE_WINDOW")


@pytest.fixture(scope="module")
def ctx2():
    """a second context: its own stream and workspaces, as another host thread's would be"""
    from ndtpso_slam_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


def _map(ctx, frame=sc.FRAME_M, og=OG_CELL, build=True):
    """(the six-scan map, the query scan) on `ctx`'s device"""
    from ndtpso_slam_amd import capi
    grid = capi.Grid(frame, frame, sc.CELL_SIDE)
    m = capi.ResidentMap(ctx, grid, og_cell_size=og, pool_bytes=POOL)
    s = capi.ResidentScan(ctx, sc.N_BEAMS)
    maps, _ = sc.ranges()
    for k, pose in enumerate(sc.MAP_POSES):
        s.load_scan(maps[k], sc.geom(), clip=grid)
        m.insert(s, np.asarray(pose, dtype=np.float64))
    if build:
        m.build()
    return m, _query(ctx, grid)


def _query(ctx, grid):
    from ndtpso_slam_amd import capi
    s = capi.ResidentScan(ctx, sc.N_BEAMS)
    s.load_scan(sc.ranges()[1], sc.geom(), clip=grid)
    return s


@pytest.fixture(scope="module")
def case(ctx, ctx2):
    """(original map, its query scan, the blob, the restored map in the second context, the query scan there)"""
    from ndtpso_slam_amd import capi
    m, s = _map(ctx)
    blob = m.snapshot()
    r = capi.ResidentMap.restore(ctx2, blob, pool_bytes=POOL)
    return m, s, blob, r, _query(ctx2, r.grid)


def snc_info(blob):
    from ndtpso_slam_amd import capi
    return capi.snapshot_describe(blob)


def _cells_key(cells):
    return [(c["index"], c["count"], c["built"], c["slot"], c["mean"].tobytes(), c["icov"].tobytes()) for c in cells]


def _assert_same_state(a, b, what=""):
    assert _cells_key(a.cells()) == _cells_key(b.cells()), what
    assert np.array_equal(a.points(), b.points()), what
    assert np.array_equal(a.points(slot0_only=True), b.points(slot0_only=True)), what
    og_a, og_b = a.occupancy(), b.occupancy()
    assert og_a[1:] == og_b[1:] and np.array_equal(og_a[0], og_b[0]), what
    ia, ib = a.info(), b.info()
    for k in ("pool_bump", "pool_free"):      # chunk ids are not state
        ia.pop(k), ib.pop(k)
    assert ia == ib, (what, ia, ib)


def _assert_same_alignment(a, sa, b, sb, modes, what=""):
    from ndtpso_slam_amd import capi
    cfg = capi.PSOConfig.make(50, 30)
    for mode in modes:
        pa, ca, sta = a.align(sa, GUESS, DEVIATION, cfg, seed=7, mode=mode)
        pb, cb, stb = b.align(sb, GUESS, DEVIATION, cfg, seed=7, mode=mode)
        assert pa.tobytes() == pb.tobytes() and struct.pack("<d", ca) == struct.pack("<d", cb), (what, mode, pa, pb, ca, cb)
        assert sta["status"] == stb["status"] and sta["n_built"] == stb["n_built"] and sta["n_points"] == stb["n_points"], (what, mode)


def test_round_trip_into_a_second_context(case):
    from ndtpso_slam_amd import capi
    m, s, blob, r, s2 = case
    _assert_same_state(m, r)
    # nothing non-zero lies outside the box the blob takes the occupancy keys from: the kernel that writes a key widens the box
    og, w, h, (x0, x1, y0, y1) = m.occupancy()
    assert w and h and x0 <= x1 and y0 <= y1
    at = np.flatnonzero(og)
    assert at.size and ((at % h >= x0) & (at % h <= x1) & (at // h >= y0) & (at // h <= y1)).all()   # og[x + height * y]
    assert snc_info(blob)["og_box_entries"] == (x1 - x0 + 1) * (y1 - y0 + 1)
    # the re-packed alignment table
    rng = np.random.default_rng(3)
    poses = np.asarray(sc.TRUTH) + rng.uniform(-1, 1, (64, 3)) * (0.5, 0.5, 0.1)
    assert np.array_equal(m.cost(s, poses, mode=capi.SCORE_F64), r.cost(s2, poses, mode=capi.SCORE_F64))
    _assert_same_alignment(m, s, r, s2, (capi.SCORE_F32, capi.SCORE_F64, capi.SCORE_EXACT))
    got_m = m.search(s, sc.ORIGIN, sc.STEP, sc.COUNT, sc.TOP_K, mode=capi.SCORE_EXACT)
    got_r = r.search(s2, sc.ORIGIN, sc.STEP, sc.COUNT, sc.TOP_K, mode=capi.SCORE_EXACT)
    for a, b in zip(got_m[:3], got_r[:3]):
        assert a.tobytes() == b.tobytes()
    assert got_m[3] == got_r[3]


def test_snapshot_of_the_restored_map_is_the_blob(case):
    m, _, blob, r, _ = case
    assert r.snapshot() == blob
    assert m.snapshot() == blob          # ... and the same state gives the same bytes again


def test_continuation_past_the_window_ring(ctx, ctx2, oracle):
    """1300 update steps (insert + build) of two scans from two alternating poses make the 100-slot ring of some cell wrap; the
    map is saved there, and 40 more steps on the original and on the restored map leave the same cells, points and alignment.
    The oracle, fed the same steps, proves the wrap and holds the device's cells before and after."""
    from ndtpso_slam_amd import capi
    from test_gpu_resident import _compare_cells
    K, MORE = 1300, 40
    grid = capi.Grid(sc.FRAME_M, sc.FRAME_M, sc.CELL_SIDE)
    maps, _ = sc.ranges()
    poses = [np.asarray(sc.MAP_POSES[2], dtype=np.float64), np.asarray(sc.MAP_POSES[3], dtype=np.float64)]
    scans, scans2, ocur = [], [], []
    for k in (2, 3):
        for c, into in ((ctx, scans), (ctx2, scans2)):
            sk = capi.ResidentScan(c, sc.N_BEAMS)
            sk.load_scan(maps[k], sc.geom(), clip=grid)
            into.append(sk)
        f = oracle.Frame((0, 0, 0), sc.FRAME_M, sc.FRAME_M, float(sc.FRAME_M))
        for q in scans[-1].get():          # (the device's points: its sincos differs from glibc's in the last ulp of a few)
            f.add_point(q[0], q[1])
        ocur.append(f)

    def cell_of(xy):
        return (np.floor((xy[:, 0] + sc.FRAME_M / 2.0) / sc.CELL_SIDE) +
                int(sc.FRAME_M / sc.CELL_SIDE) * np.floor((xy[:, 1] + sc.FRAME_M / 2.0) / sc.CELL_SIDE)).astype(np.int64)

    n_cells = int(sc.FRAME_M / sc.CELL_SIDE) ** 2
    per_step = []
    for j in range(2):                       # points one step of scan j puts into each cell, by the oracle's own update
        probe = oracle.Frame((0, 0, 0), sc.FRAME_M, sc.FRAME_M, sc.CELL_SIDE)
        probe.update(poses[j], ocur[j])
        per_step.append(np.bincount(cell_of(probe.points_all()), minlength=n_cells))

    m = capi.ResidentMap(ctx, grid, pool_bytes=POOL)
    ref = oracle.Frame((0, 0, 0), sc.FRAME_M, sc.FRAME_M, sc.CELL_SIDE)

    def step(k, device):
        for mm, ss in device:
            mm.insert(ss[k % 2], poses[k % 2])
            mm.build()
        ref.update(poses[k % 2], ocur[k % 2])
        ref.build()

    for k in range(K):
        step(k, [(m, scans)])
    stored = np.bincount(cell_of(ref.points_all()), minlength=n_cells)
    inserted = per_step[0] * ((K + 1) // 2) + per_step[1] * (K // 2)
    assert (stored <= inserted).all()
    wrapped = np.flatnonzero(stored < inserted)
    assert wrapped.size >= 1, "no cell's ring has wrapped after %d steps" % K
    _compare_cells(m.cells(), ref.cells())
    assert np.array_equal(m.points(), ref.points_all())

    r = capi.ResidentMap.restore(ctx2, m.snapshot(), pool_bytes=POOL)
    _assert_same_state(m, r, "at the save")
    for k in range(K, K + MORE):
        step(k, [(m, scans), (r, scans2)])
    _assert_same_state(m, r, "40 steps on")
    _compare_cells(r.cells(), ref.cells())
    assert np.array_equal(r.points(), ref.points_all())
    _assert_same_alignment(m, _query(ctx, grid), r, _query(ctx2, grid), (capi.SCORE_EXACT,), "40 steps on")


def test_unbuilt_and_speculative_states(ctx, ctx2):
    from ndtpso_slam_amd import capi
    # points inserted since the last build (here: never built): saved unbuilt, the lazy build gives what the original's gives
    m, s = _map(ctx, build=False)
    blob = m.snapshot()
    assert snc_info(blob)["built"] == 0
    r = capi.ResidentMap.restore(ctx2, blob, pool_bytes=POOL)
    s2 = _query(ctx2, r.grid)
    _assert_same_alignment(m, s, r, s2, (capi.SCORE_EXACT,), "unbuilt")
    _assert_same_state(m, r, "after the lazy build")
    # a built map, one more scan inserted: the blob of the settled map, and the blob after a speculative build, which the
    # snapshot puts back first
    maps, _ = sc.ranges()
    extra = capi.ResidentScan(ctx, sc.N_BEAMS)
    extra.load_scan(maps[0], sc.geom(), clip=m.grid)
    m.insert(extra, np.array([0.5, 0.25, 0.1]))
    settled = m.snapshot()
    assert snc_info(settled)["built"] == 0
    m.speculate_build()
    assert m.snapshot() == settled
    # ... and the original aligns afterwards as if nothing had happened
    twin = capi.ResidentMap.restore(ctx2, settled, pool_bytes=POOL)
    _assert_same_alignment(m, s, twin, s2, (capi.SCORE_EXACT,), "after a speculation that was put back")
    _assert_same_state(m, twin, "after a speculation that was put back")


def test_the_restored_map_is_independent(case, ctx2):
    from ndtpso_slam_amd import capi
    m, _, blob, _, _ = case
    before = _cells_key(m.cells())
    r = capi.ResidentMap.restore(ctx2, blob, pool_bytes=POOL)
    extra = capi.ResidentScan(ctx2, sc.N_BEAMS)
    extra.load_scan(sc.ranges()[0][1], sc.geom(), clip=r.grid)
    r.insert(extra, np.array([-1.0, 0.5, 0.3]))
    r.build()
    assert _cells_key(r.cells()) != before
    assert _cells_key(m.cells()) == before
    assert m.snapshot() == blob


def test_size_follows_content_not_the_frame(case, ctx):
    m, _, blob, _, _ = case
    info = snc_info(blob)
    assert info["bytes"] == len(blob) <= snc.size_bound(info), (len(blob), snc.size_bound(info), info)
    assert info["n_created"] == m.info()["n_created"] and info["n_points_stored"] == len(m.points())
    # the same six scans in a 120 m frame (same cell boundaries): everything before the occupancy keys is no larger
    big, _ = _map(ctx, frame=2 * sc.FRAME_M)
    big_blob = big.snapshot()
    big_info = snc_info(big_blob)
    assert snc.section_offsets(big_blob)["og"] <= snc.section_offsets(blob)["og"]
    assert len(big_blob) <= snc.size_bound(big_info)
    for k in ("n_created", "n_slots_used", "n_chunks", "n_points_stored"):
        assert big_info[k] == info[k], k


def test_empty_and_non_square_maps(ctx, ctx2):
    """a map nothing was inserted into is a header alone; a frame that is wider than high keeps the reference's occupancy
    indexing (og[x + height * y] with the row taken from index / heightNumOfCells), box and all"""
    from ndtpso_slam_amd import capi
    empty = capi.ResidentMap(ctx, capi.Grid(20, 20, 1.0), og_cell_size=0.25, pool_bytes=1 << 20)
    blob = empty.snapshot()
    info = snc_info(blob)
    assert len(blob) == snc.HEADER_BYTES and info["n_created"] == 0 and info["n_chunks"] == 0 and info["og_box_entries"] == 0
    r = capi.ResidentMap.restore(ctx2, blob, pool_bytes=1 << 20)
    assert r.snapshot() == blob and r.cells() == [] and r.info()["n_points"] == 0
    grid = capi.Grid(sc.FRAME_M, 40, sc.CELL_SIDE)
    m = capi.ResidentMap(ctx, grid, og_cell_size=OG_CELL, pool_bytes=POOL)
    s = capi.ResidentScan(ctx, sc.N_BEAMS)
    for k, pose in enumerate(sc.MAP_POSES):
        s.load_scan(sc.ranges()[0][k], sc.geom(), clip=grid)
        m.insert(s, np.asarray(pose, dtype=np.float64))
    m.build()
    blob = m.snapshot()
    assert snc_info(blob)["og_box_entries"] > 0 and len(blob) <= snc.size_bound(snc_info(blob))
    r = capi.ResidentMap.restore(ctx2, blob, pool_bytes=POOL)
    _assert_same_state(m, r, "60 m x 40 m")
    assert r.snapshot() == blob


def _restore_raw(ctx, blob, pool=POOL):
    h = C.c_void_p()
    rc = ctx._lib.ndtpso_map_restore(ctx._h, blob, len(blob), pool, C.byref(h))
    return rc, h.value, ctx._lib.ndtpso_last_error(ctx._h).decode()


def test_refusals_leave_nothing_behind(case, ctx2):
    from ndtpso_slam_amd import capi
    m, _, blob, _, _ = case
    off = snc.section_offsets(blob)
    flipped = bytearray(blob)
    flipped[off["cells"] + 40] ^= 0x10
    cases = [(blob[:off[k]], "bytes") for k in ("cells", "win_sum", "chunks")]
    cases += [(bytes(flipped), "checksum"),
              (snc.reseal(b"XDTPSOMP" + blob[8:]), "magic"),
              (snc.with_u32(blob, snc.VERSION, 2), "version"),
              (snc.with_u32(blob, snc.WINDOW_SIZE, 99), "NDTPSO_WINDOW_SIZE")]
    for bad, field in cases:
        rc, handle, err = _restore_raw(ctx2, bad)
        assert rc == capi.E_ARG and handle is None and field in err, (field, rc, handle, err)
    # a pool too small for the blob's chunks
    assert snc_info(blob)["n_chunks"] > 64
    rc, handle, err = _restore_raw(ctx2, blob, pool=64 * 512)
    assert rc == capi.E_CAPACITY and handle is None and "pool_bytes" in err, (rc, handle, err)
    # a buffer one byte short: the size needed comes back, nothing is written
    n = C.c_uint64()
    buf = C.create_string_buffer(len(blob))
    rc = m._lib.ndtpso_map_snapshot(m._h, buf, len(blob) - 1, C.byref(n))
    assert rc == capi.E_CAPACITY and n.value == len(blob) and buf.raw == bytes(len(blob))
    assert "capacity" in m._lib.ndtpso_last_error(m._ctx._h).decode()
    # a valid restore still works afterwards
    r = capi.ResidentMap.restore(ctx2, blob, pool_bytes=POOL)
    assert r.snapshot() == blob


def test_pinned_format(ctx, oracle):
    """tests/golden/map_snapshot_v1.bin (made by tests/golden/make_golden_snapshot.py) restores today, to the cells the oracle
    builds from the same scan; its own snapshot is the pinned blob byte for byte, and a map made today from that scan holds the
    same cells, points and counts."""
    from ndtpso_slam_amd import capi
    from test_gpu_resident import _compare_cells
    blob = open(snc.GOLDEN, "rb").read()
    r = capi.ResidentMap.restore(ctx, blob, pool_bytes=1 << 20)
    m, s = snc.golden_map(ctx)
    ref = oracle.Frame((0, 0, 0), snc.GOLDEN_FRAME_M, snc.GOLDEN_FRAME_M, snc.GOLDEN_CELL_SIDE)
    for q in s.get():
        ref.add_point(q[0], q[1])
    ref.build()
    assert len(ref.cells()) > 20 and any(c["built"] for c in ref.cells())
    _compare_cells(r.cells(), ref.cells())
    assert np.array_equal(r.points(), ref.points_all())
    assert r.snapshot() == blob
    # today's map of the same scan holds the same state (its blob may list the cells one insert created in another order:
    # they enter created[] as the insert's atomics land)
    assert _cells_key(m.cells()) == _cells_key(r.cells()) and np.array_equal(m.points(), r.points())
    assert snc_info(m.snapshot()) == snc_info(blob)
    with open(snc.GOLDEN_INFO) as f:
        assert json.loads(json.dumps(snc_info(blob))) == json.load(f)


# ---- the drop-in, across processes ------------------------------------------------------------------------------------------------
N_SCANS = 40
SEED0 = 100


@pytest.fixture(scope="module")
def scans(tmp_path_factory):
    from ndtpso_slam_amd import synth
    from test_gpu_resident import _trajectory
    path = tmp_path_factory.mktemp("snapshot") / "scans.bin"
    with open(path, "wb") as f:
        np.array([N_SCANS, synth.N_BEAMS], dtype=np.int32).tofile(f)
        np.array([synth.ANGLE_MIN, synth.ANGLE_INC, synth.RANGE_MAX], dtype=np.float32).tofile(f)
        _trajectory(N_SCANS).tofile(f)
    return path


def _check(scans, env, *mode):
    args = [EXE, str(scans), str(sc.FRAME_M), repr(sc.CELL_SIDE), str(SEED0)] + [str(a) for a in mode]
    r = subprocess.run(args, text=True, capture_output=True, env=env, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[-2000:])
    return r.stdout.splitlines()


@pytest.mark.parametrize("score", ["exact", "f64"])
def test_a_saved_frame_resumes_in_another_process(scans, tmp_path, score):
    env = dict({k: v for k, v in os.environ.items() if k not in ENV_OFF}, NDTPSO_SCORE=score)
    straight = [l for l in _check(scans, env, "straight", N_SCANS) if l.startswith("pose ")]
    assert len(straight) == N_SCANS
    file = tmp_path / "frame.ndt"
    first = _check(scans, env, "save", N_SCANS // 2, file)
    assert first[:-1] == straight[:N_SCANS // 2] and first[-1].split()[:4] == ["saved", "1", "errors", "0"], first[-1]
    assert file.exists() and not os.path.exists(str(file) + ".tmp")
    resumed = _check(scans, env, "resume", file, N_SCANS)
    assert resumed == straight[N_SCANS // 2:]
    assert len(set(straight)) == N_SCANS          # (the poses move: the comparison is not of forty equal lines)


def test_save_of_a_frame_that_is_not_resident_fails_loudly(scans, tmp_path):
    env = dict({k: v for k, v in os.environ.items() if k not in ENV_OFF + ("NDTPSO_ABORT_ON_ERROR",)}, NDTPSO_RESIDENT="0")
    file = tmp_path / "frame.ndt"
    out = _check(scans, env, "save", 2, file)
    w = out[-1].split()
    assert w[:4] == ["saved", "0", "errors", "1"] and "not resident" in out[-1], out[-1]
    assert not file.exists() and not os.path.exists(str(file) + ".tmp")
