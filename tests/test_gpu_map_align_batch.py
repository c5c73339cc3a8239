"""ndtpso_map_align_batch / capi.align_maps: several ndtpso_map_align calls of one context in ONE launch (k_align_jobs).

The contract is the single call's: every job's pose, cost, status, n_points, n_built and gbest_updates are bit for bit what
ResidentMap.align returns for the same arguments -- whatever mixture of maps (grids, windows, table sizes), rand() sources and
score modes the jobs are, and whether the launch runs them on one workgroup or on a cluster of workgroups each -- and the maps
end up in the state the single calls would leave them in.  The reference here is therefore ResidentMap.align, job by job, on
the same maps in the same process BEFORE the batch call (an alignment does not change a built map); the first test also ties
job 0 to the CPU oracle."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import FRAME_M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = (0.1, 0.1, 3.1415e-3)


def _rel(p0, p):
    """pose p in the frame of pose p0"""
    c, s = np.cos(p0[2]), np.sin(p0[2])
    dx, dy = p[0] - p0[0], p[1] - p0[1]
    return np.array([c * dx + s * dy, -s * dx + c * dy, p[2] - p0[2]])


def _trajectory(n_scans, start, seed, step=0.6):
    """tests/test_gpu_resident.py::_trajectory from another place of the world: (ranges [n, beams], poses in scan 0's frame)"""
    from ndtpso_slam_amd import synth
    rng = np.random.default_rng(seed)
    s = np.linspace(0.0, step, n_scans)
    poses = np.stack([start[0] + 1.2 * s, start[1] + 0.8 * np.sin(1.5 * s), start[2] + 0.25 * s], axis=1)
    clean = synth.raycast(poses)
    ranges = np.where(clean > 0, clean + rng.normal(0, 0.01, clean.shape), 0.0).astype(np.float32)
    return ranges, np.stack([_rel(poses[0], p) for p in poses])


def _geom():
    from ndtpso_slam_amd import capi, synth
    return capi.ScanGeom(synth.N_BEAMS, synth.ANGLE_MIN, synth.ANGLE_INC, synth.RANGE_MAX, 0.1)


class _World:
    """Maps of 3 - 4 inserted scans each (two 60 m / 0.5 m maps built at different places of the world: windows and table
    sizes differ; one 60 m / 0.25 m map: the grid differs; a third 0.5 m map for the tests that want three maps whose windows
    can be bound late -- the 0.25 m map's is not: planned for the whole grid its table is not the dense form, so it waits for
    its header) and, per map, the next scan of its trajectory loaded on the device."""

    SPECS = [((2.0, -1.0, 0.3), 0.5, 4, 4), ((-6.0, 3.0, -0.8), 0.5, 3, 9), ((4.0, 4.0, 2.0), 0.25, 4, 13),
             ((-3.0, -5.0, 1.1), 0.5, 3, 17)]

    def __init__(self, ctx, og_cell_size=0.0):
        from ndtpso_slam_amd import capi, synth
        self.ctx, self.geom = ctx, _geom()
        self.maps, self.scans, self.guess, self.inserted = [], [], [], []
        for start, cs, n_ins, seed in self.SPECS:
            ranges, poses = _trajectory(n_ins + 1, start, seed)
            grid = capi.Grid(FRAME_M, FRAME_M, cs)
            m = capi.ResidentMap(ctx, grid, og_cell_size=og_cell_size, pool_bytes=64 << 20)
            scan = capi.ResidentScan(ctx, synth.N_BEAMS)
            pts = []
            for k in range(n_ins):
                scan.load_scan(ranges[k], self.geom, clip=grid)
                pts.append((scan.get(), poses[k].copy()))
                m.insert(scan, poses[k])
            scan.load_scan(ranges[n_ins], self.geom, clip=grid)
            self.maps.append(m)
            self.scans.append(scan)
            self.guess.append(poses[n_ins - 1].copy())     # the node's guess: the previous pose
            self.inserted.append(pts)

    def jobs9(self, n_draw):
        """Nine jobs (a second cluster per XCD slot): map 0 four times with different guesses and seeds, map 1 three times,
        map 2 twice; host tables for jobs 0, 3, 5 and 8, the device's replay of srand(seed) for the others."""
        rng = np.random.default_rng(99)
        which = [0, 1, 2, 0, 1, 0, 2, 0, 1]
        jobs = []
        for j, w in enumerate(which):
            g = self.guess[w] + (0.0 if j < 3 else 1.0) * np.array([0.03 * np.cos(j), 0.03 * np.sin(j), 0.004 * (j - 4)])
            src = rng.integers(0, 2 ** 31 - 1, size=n_draw).astype(np.int32) if j in (0, 3, 5, 8) else 1000 + j
            jobs.append((self.maps[w], self.scans[w], g, DEV, src))
        return jobs


@pytest.fixture(scope="module")
def world(ctx):
    return _World(ctx)


def _single(jobs, cfg, mode):
    """the reference: ResidentMap.align, job by job"""
    out = []
    for m, scan, g, d, src in jobs:
        kw = dict(seed=int(src)) if isinstance(src, (int, np.integer)) else dict(rand_table=src)
        out.append(m.align(scan, g, d, cfg, mode=mode, **kw))
    return out


def _assert_equal(got, want, what=""):
    poses, costs, st, rc, route = got
    assert (rc == 0).all(), (what, rc)
    for j, (p, c, s) in enumerate(want):
        assert np.array_equal(poses[j], p) and costs[j] == c, (what, j, poses[j], p, costs[j], c, route[j])
        for k in ("status", "n_points", "n_built", "gbest_updates"):
            assert int(st[k][j]) == int(s[k]), (what, j, k, int(st[k][j]), s[k])


def _n_draw(cfg):
    return 3 + 3 * cfg.population + 6 * cfg.population * cfg.iterations


@pytest.mark.parametrize("shape", [(30, 50), (70, 12), (5, 8)])       # (population, iterations): the live shape on clusters with
def test_mixed_jobs_equal_the_single_calls(ctx, world, oracle, shape):  # SpecP; 8-wave cluster workgroups without; never a cluster
    from ndtpso_slam_amd import capi
    P, I = shape
    cfg = capi.PSOConfig.make(I, P)
    jobs = world.jobs9(_n_draw(cfg))
    for mode in (capi.SCORE_F64, capi.SCORE_F32, capi.SCORE_EXACT):
        want = _single(jobs, cfg, mode)
        got = capi.align_maps(ctx, jobs, cfg, mode)
        _assert_equal(got, want, (shape, mode))
        route = got[4]
        # 0.5 m and 0.25 m cells, a room's worth of built cells, swarms that fit LDS: the dense form (fp32 score, exact mode) and
        # the fp64 score's bitmap of power-of-two cells -- every job has a job kernel, so a loop over the single call cannot pass
        assert (route >= 1).all(), (shape, mode, route)
        if shape == (30, 50):
            assert (route >= 2).all(), (mode, route)        # nine jobs, 256 compute units: a cluster each
        if shape == (5, 8):
            assert (route == 1).all(), (mode, route)        # six items: one workgroup already has a wave per item
        if mode == capi.SCORE_F64 and shape == (30, 50):
            # job 0 against the CPU oracle: the same points (the device's), the same table of draws
            m, scan, g, d, table = jobs[0]
            ref = oracle.Frame((0, 0, 0), FRAME_M, FRAME_M, world.SPECS[0][1])
            for pts, pose in world.inserted[0]:
                cur = oracle.Frame((0, 0, 0), FRAME_M, FRAME_M, float(FRAME_M))
                for q in pts:
                    cur.add_point(q[0], q[1])
                ref.update(pose, cur)
            new = oracle.Frame((0, 0, 0), FRAME_M, FRAME_M, float(FRAME_M))
            for q in scan.get():
                new.add_point(q[0], q[1])
            opose, _, _ = ref.pso(g, new, np.array(d), oracle.PSOConfig.make(I, P), table=table)
            assert np.abs(got[0][0] - opose).max() < 1e-9, (got[0][0], opose)


def test_two_jobs_and_seventy_jobs_on_one_map(ctx, world):
    from ndtpso_slam_amd import capi
    m, scan, g0 = world.maps[0], world.scans[0], world.guess[0]
    for mode in (capi.SCORE_EXACT, capi.SCORE_F64):
        cfg = capi.PSOConfig.make(50, 30)
        two = [(m, scan, g0, DEV, 5), (m, scan, g0, DEV, 5)]              # the smallest batch that reaches the kernel
        got = capi.align_maps(ctx, two, cfg, mode)
        _assert_equal(got, _single(two, cfg, mode), ("two", mode))
        assert (got[4] >= 1).all(), got[4]
        cfg = capi.PSOConfig.make(10, 30)
        many = [(m, scan, g0 + np.array([0.002 * (j % 9), -0.003 * (j % 7), 0.0005 * (j % 5)]), DEV, 300 + j) for j in range(70)]
        got = capi.align_maps(ctx, many, cfg, mode)
        _assert_equal(got, _single(many, cfg, mode), ("seventy", mode))
        # one workgroup per job: 70 alignments in flight are past the cap of 16 beyond which the library forms no clusters (as
        # for any call of 17 jobs or more); launch_pairs' rules alone would say the same (256 / 70 = 3 workgroups of 4 waves)
        assert (got[4] == 1).all(), got[4]


def _speculative_pair(ctx, which=(0, 1, 2, 3)):
    """Two identical worlds whose maps each have a speculative build in flight behind a header the host knows (insert x n,
    align, insert, speculate_build): (batch world, twin world, jobs of each)."""
    from ndtpso_slam_amd import capi
    cfg = capi.PSOConfig.make(50, 30)
    worlds = []
    for _ in range(2):
        w = _World(ctx, og_cell_size=0.1)
        for m, scan, g in zip(w.maps, w.scans, w.guess):
            pose, _, _ = m.align(scan, g, DEV, cfg, seed=3, mode=capi.SCORE_EXACT)     # lazy build; the header reaches the host
            m.insert(scan, pose)
            m.speculate_build()
        worlds.append(w)
    jobs = [[(w.maps[k], w.scans[k], w.guess[k], DEV, 40 + k) for k in which] for w in worlds]
    return worlds[0], worlds[1], jobs[0], jobs[1], cfg


def _same_maps(a, b):
    for ma, mb in zip(a.maps, b.maps):
        ca, cb = ma.cells(), mb.cells()
        assert len(ca) == len(cb)
        for x, y in zip(ca, cb):
            assert x["index"] == y["index"] and x["count"] == y["count"] and x["built"] == y["built"] and x["slot"] == y["slot"]
            assert np.array_equal(x["mean"], y["mean"], equal_nan=True) and np.array_equal(x["icov"], y["icov"], equal_nan=True)
        assert np.array_equal(ma.points(), mb.points())
        oa, ob = ma.occupancy(), mb.occupancy()
        assert oa[1:] == ob[1:] and np.array_equal(oa[0], ob[0])


def test_behind_a_speculative_build(ctx):
    """The launch is enqueued before any header has reached the host (late window binding); poses equal the single calls' on
    twin maps, and afterwards cells, points and occupancy grids of the maps are the twins'."""
    from ndtpso_slam_amd import capi
    wa, wb, ja, jb, cfg = _speculative_pair(ctx)
    got = capi.align_maps(ctx, ja, cfg, capi.SCORE_EXACT)
    _assert_equal(got, _single(jb, cfg, capi.SCORE_EXACT), "speculative")
    assert (got[4] >= 1).all(), got[4]
    _same_maps(wa, wb)


CHILD_REDO = r"""
import json, sys
import numpy as np
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import test_gpu_map_align_batch as t
from ndtpso_slam_amd import capi
ctx = capi.Context(0)
wa, wb, ja, jb, cfg = t._speculative_pair(ctx, which=(0, 1, 3))     # J = 3, every map's window bound late
got = capi.align_maps(ctx, ja, cfg, capi.SCORE_EXACT)
t._assert_equal(got, t._single(jb, cfg, capi.SCORE_EXACT), "redo")
t._same_maps(wa, wb)
print(json.dumps(dict(route=[int(r) for r in got[4]])))
"""


def _run_child(script, env_extra=None, lib=None):
    env = {k: v for k, v in os.environ.items() if k not in ("NDTPSO_LIB", "NDTPSO_EXACT_CHECK", "NDTPSO_LATE_TEST_OVERFLOW")}
    env.update(env_extra or {})
    if lib:
        env["NDTPSO_LIB"] = lib
    r = subprocess.run([sys.executable, "-c", script % dict(root=ROOT, tests=os.path.join(ROOT, "tests"))], capture_output=True,
                       text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return json.loads(r.stdout.strip().splitlines()[-1]), r.stderr


def test_a_job_whose_late_bound_window_overflows_is_redone_alone():
    """NDTPSO_LATE_TEST_OVERFLOW=1: every job of the launch behind the speculative builds comes back with the overflow flag and
    is redone through the single path -- route 0, the twin's pose, the twin's map."""
    d, _ = _run_child(CHILD_REDO, {"NDTPSO_LATE_TEST_OVERFLOW": "1"})
    assert d["route"] == [0, 0, 0], d


CHILD_CHECK = r"""
import json, sys
import numpy as np
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import test_gpu_map_align_batch as t
from ndtpso_slam_amd import capi
ctx = capi.Context(0)
before = ctx.exact_check_report()["job_families"]
w = t._World(ctx)
cfg = capi.PSOConfig.make(50, 30)
jobs = w.jobs9(t._n_draw(cfg))
px = capi.align_maps(ctx, jobs, cfg, capi.SCORE_EXACT)
err = ctx._lib.ndtpso_last_error(ctx._h).decode()
p64 = capi.align_maps(ctx, jobs, cfg, capi.SCORE_F64)
rep = ctx.exact_check_report()
print(json.dumps(dict(before=before, report=rep, state=ctx.exact_check_jobs(), err=err,
                      equal=bool(np.array_equal(px[0], p64[0]) and np.array_equal(px[1], p64[1])),
                      arbitrated=int(px[2]["arbitrated"].sum()), route=[int(r) for r in px[4]])))
"""


def test_the_exact_mode_checks_its_job_kernels_before_it_trusts_them():
    d, _ = _run_child(CHILD_CHECK)
    assert d["before"] == [], d["before"]                 # empty until the check has run
    fam = d["report"]["job_families"]
    assert len(fam) == 2 and d["state"] == 1, d
    for f in fam:
        assert f["state"] == "passed" and f["launched"] == f["instantiation"] and f["arbitrated"] > 0 and f["mismatched"] == 0, f
    assert len(d["report"]["families"]) == 16
    assert d["equal"] and min(d["route"]) >= 2, d


def test_a_library_with_a_broken_arbitration_is_refused_the_exact_mode_for_jobs_too():
    from ndtpso_slam_amd import build
    lib = build.variant_path("broken")
    if not os.path.exists(lib):
        pytest.skip("the -DNDTPSO_BREAK_ARBITRATION variant was not built (python -m ndtpso_slam_amd.build broken)")
    d, stderr = _run_child(CHILD_CHECK, lib=lib)
    fam = d["report"]["job_families"]
    assert len(fam) == 2 and d["state"] == 2, d
    for f in fam:
        assert f["state"] == "refused" and f["launched"] == f["instantiation"], f
    assert "refused" in d["err"] and "refused" in stderr, (d["err"], stderr[-500:])
    # ... and the batch entry's exact-mode results are the fp64 mode's, from the fp64 kernels: nothing arbitrated
    assert d["equal"] and d["arbitrated"] == 0, d


def test_errors(ctx, world):
    from ndtpso_slam_amd import capi, synth
    cfg = capi.PSOConfig.make(50, 30)
    other = capi.Context(0)
    try:
        foreign = capi.ResidentScan(other, synth.N_BEAMS)
        bad = [(world.maps[0], world.scans[0], world.guess[0], DEV, 1), (world.maps[1], foreign, world.guess[1], DEV, 2)]
        with pytest.raises(capi.NdtpsoError) as e:
            capi.align_maps(ctx, bad, cfg, capi.SCORE_EXACT)            # a scan of another context: nothing runs
        assert e.value.code == capi.E_ARG
        foreign.close()
    finally:
        other.close()
    with pytest.raises(capi.NdtpsoError) as e:
        capi.align_maps(ctx, [], cfg, capi.SCORE_EXACT)
    assert e.value.code == capi.E_ARG
    # one job on a map whose point pool has run out (a pool that cannot grow): its rc says so, the others complete
    os.environ["NDTPSO_MAP_POOL_FIXED"] = "1"
    try:
        fixed = capi.ResidentMap(ctx, capi.Grid(FRAME_M, FRAME_M, 0.5), pool_bytes=64 * 512)
        fixed.insert(world.scans[0], (0, 0, 0))
        jobs = [(world.maps[0], world.scans[0], world.guess[0], DEV, 7), (fixed, world.scans[0], (0, 0, 0), DEV, 8),
                (world.maps[2], world.scans[2], world.guess[2], DEV, 9)]
        want = _single([jobs[0], jobs[2]], cfg, capi.SCORE_EXACT)
        poses, costs, st, rc, route = capi.align_maps(ctx, jobs, cfg, capi.SCORE_EXACT)
    finally:
        del os.environ["NDTPSO_MAP_POOL_FIXED"]
    assert list(rc) == [0, capi.E_CAPACITY, 0], rc
    for j, (p, c, _) in zip((0, 2), want):
        assert np.array_equal(poses[j], p) and costs[j] == c and route[j] >= 1, (j, poses[j], p, route)
