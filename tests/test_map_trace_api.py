"""ndtpso_map_trace / ndtpso_map_trace_batch / ndtpso_map_get_trace_info / ndtpso_map_get_trace / ndtpso_map_get_nav_grid without a
device: the C-ABI's structures against the header's defines, the symbols and their bindings, the traversal rule's restatement
(tests/trace_ref.py) against geometry, the nav grid's rule, and the replay tool in the host library's build."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np

import trace_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRACE_EXPORTS = (("ndtpso_map_trace", 3), ("ndtpso_map_trace_batch", 3), ("ndtpso_map_get_trace_info", 2), ("ndtpso_map_get_trace", 4),
                 ("ndtpso_map_get_nav_grid", 3))


def _define(header, name):
    m = re.search(r"#define %s (\d+)\b" % name, header)
    assert m, name
    return int(m.group(1))


def test_struct_sizes_and_offsets_match_the_header():
    from ndtpso_slam_amd import capi
    header = open(os.path.join(ROOT, "include", "ndtpso_hip.h")).read()
    job, info = capi.MapTraceJob, capi.TraceInfo
    assert C.sizeof(job) == _define(header, "NDTPSO_MAP_TRACE_JOB_BYTES") == 48
    assert job.map.offset == 0 and job.points.offset == 8
    assert job.pose.offset == _define(header, "NDTPSO_MAP_TRACE_JOB_POSE_OFFSET") == 16
    assert job.rc.offset == _define(header, "NDTPSO_MAP_TRACE_JOB_RC_OFFSET") == 40
    assert job.reserved.offset == 44
    assert C.sizeof(info) == _define(header, "NDTPSO_TRACE_INFO_BYTES") == 56
    assert info.allocated.offset == 0 and info.width.offset == 4 and info.height.offset == 8
    assert info.extent.offset == _define(header, "NDTPSO_TRACE_INFO_EXTENT_OFFSET") == 16
    assert info.n_rays.offset == _define(header, "NDTPSO_TRACE_INFO_N_RAYS_OFFSET") == 32
    assert info.n_skipped.offset == 40 and info.n_steps.offset == 48
    for name in ("ndtpso_map_trace_job", "ndtpso_trace_info"):   # the header asserts the same sizes to a C and a C++ compiler
        assert "static_assert(sizeof(%s) == " % name in header
        assert "_Static_assert(sizeof(%s) == " % name in header


def test_symbols_are_exported_and_bound():
    from ndtpso_slam_amd import capi
    L = capi.load()
    for name, n_args in TRACE_EXPORTS:
        assert name in capi.EXPORTS
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == n_args
        assert fn.restype is C.c_int
    assert callable(capi.trace_maps)
    for member in ("trace", "trace_info", "trace_counts", "nav_grid"):
        assert callable(getattr(capi.ResidentMap, member))
    # null handles are refused before anything touches a device
    assert L.ndtpso_map_trace(None, None, None) == capi.E_ARG
    assert L.ndtpso_map_trace_batch(None, None, 0) == capi.E_ARG
    assert L.ndtpso_map_get_trace_info(None, None) == capi.E_ARG
    assert L.ndtpso_map_get_trace(None, None, None, 0) == capi.E_ARG
    assert L.ndtpso_map_get_nav_grid(None, None, 0) == capi.E_ARG


def test_kernel_is_a_unit_of_its_own():
    units = open(os.path.join(ROOT, "ndtpso_slam_amd", "csrc", "hip_units.txt")).read().split()
    assert "ndtpso_map_trace.hip" in units
    for f in ("ndtpso_map_trace.hip", "ndtpso_map_trace.h", "ndtpso_map_trace.inc"):
        assert os.path.exists(os.path.join(ROOT, "ndtpso_slam_amd", "csrc", f))


# ---- the traversal rule against geometry: 3000 random, axis-parallel and corner-hitting rays on a 60 m / 0.25 m grid ---------------

def _rays():
    rng = np.random.default_rng(0)
    cs = 0.25
    for it in range(3000):
        o = rng.uniform(-29, 29, 2)
        e = o + rng.uniform(-1, 1, 2) * rng.choice([0.01, 1, 20])
        if it % 7 == 0:
            e[0] = o[0]
        if it % 11 == 0:
            e[1] = o[1]
        if it % 13 == 0:   # origin at a cell centre, offsets of whole cells on both axes: exactly representable ties
            o = np.round(o / cs) * cs + cs / 2
            e = o + np.array([rng.integers(-9, 9), 0]) * cs + np.array([1, 1]) * cs * rng.integers(-8, 8)
        yield o, np.clip(e, -29.9, 29.9)


def test_traversal_against_geometry():
    hw = hh = 30.0
    cs = 0.25
    worst, missed, total, ties = 0.0, 0, 0, 0
    for o, e in _rays():
        cells = tr.ray_cells((float(o[0]), float(o[1])), (float(e[0]), float(e[1])), hw, hh, cs)
        ix, iy, jx, jy, sx, sy, nx, ny, tx0, tdx, ty0, tdy = tr.ray_setup(o, e, hw, hh, cs)
        # the cell count is nx + ny + 1, no repeats, from the origin's cell to the end's, one axis step at a time
        assert len(cells) == nx + ny + 1 and len(set(cells)) == len(cells)
        assert cells[0] == (ix, iy) and cells[-1] == (jx, jy)
        assert all(abs(a[0] - b[0]) + abs(a[1] - b[1]) == 1 for a, b in zip(cells, cells[1:]))
        total += len(cells)
        a, b = (o + hw) / cs, (e + hw) / cs
        d = b - a
        L2 = float(d @ d)
        # the centre of every visited cell lies within sqrt(0.5) cells of the segment
        for cx, cy in cells:
            c = np.array([cx + 0.5, cy + 0.5])
            t = 0.0 if L2 == 0 else min(1.0, max(0.0, float((c - a) @ d) / L2))
            worst = max(worst, float(np.linalg.norm(a + t * d - c)))
        # no sampled point deeper than 0.02 cells inside a cell lies in an unvisited cell
        if L2 > 0:
            ts = np.linspace(0, 1, int(math.sqrt(L2) * 8) + 2)
            pts = a[None] + ts[:, None] * d[None]
            fr = pts - np.floor(pts)
            deep = np.minimum(fr, 1 - fr).min(axis=1) > 0.02
            S = set(cells)
            missed += sum((int(p[0]), int(p[1])) not in S for p in np.floor(pts[deep]).astype(int))
        if nx and ny and tx0 == ty0:
            ties += 1
            assert cells[1] == (ix + sx, iy)          # a tie steps x first
    print("cells", total, "worst centre distance", worst, "deep samples outside the visited set", missed, "rays with a tie at the first crossing", ties)
    assert worst <= math.sqrt(0.5) + 1e-9
    assert missed == 0
    assert ties > 20       # the corner-hitting rays of the recipe do hit corners


def test_hand_made_rays():
    hw = hh = 30.0
    cs = 0.25
    c0 = (0.125, 0.125)   # the centre of cell (120, 120)
    assert tr.ray_cells(c0, c0, hw, hh, cs) == [(120, 120)]                                       # zero length: the hit alone
    assert tr.ray_cells(c0, (0.125 + 3 * cs, 0.125), hw, hh, cs) == [(120 + i, 120) for i in range(4)]   # dy == 0
    assert tr.ray_cells(c0, (0.125, 0.125 - 2 * cs), hw, hh, cs) == [(120, 120 - j) for j in range(3)]   # dx == 0
    for sx in (1, -1):                                                                             # through exact corners
        for sy in (1, -1):
            cells = tr.ray_cells(c0, (0.125 + sx * 2 * cs, 0.125 + sy * 2 * cs), hw, hh, cs)
            assert cells == [(120, 120), (120 + sx, 120), (120 + sx, 120 + sy), (120 + 2 * sx, 120 + sy), (120 + 2 * sx, 120 + 2 * sy)]
    assert tr.ray_cells(c0, (0.5, 0.125), hw, hh, cs)[-1] == (122, 120)                          # an end exactly on a border: the upper cell
    assert tr.ray_cells(c0, (30.0, 0.0), hw, hh, cs) is None and tr.ray_cells((0.0, -30.0), c0, hw, hh, cs) is None
    assert tr.ray_cells(c0, (29.999, 0.0), hw, hh, cs)[-1] == (239, 120)


def test_counters_and_nav_grid_rule():
    cnt = tr.Counters(60, 60, 0.25)
    xy = np.array([[1.0, 0.0], [1.0, 0.0], [0.0, 0.0], [100.0, 0.0]])
    cnt.trace(xy, (0.125, 0.125, 0.0), 1.0, 0.0)
    hits, passes = cnt.grids()
    assert (cnt.n_rays, cnt.n_skipped, cnt.n_steps) == (3, 1, 8)
    assert hits.sum() == 3 and passes.sum() == 8
    assert hits[120, 124] == 2 and hits[120, 120] == 1 and passes[120, 120] == 2 and passes[120, 123] == 2
    assert cnt.extent == [120, 124, 120, 120]
    assert steps_equal(xy, (0.125, 0.125, 0.0), cnt)
    occ = np.zeros((240, 240), dtype=np.int8)
    occ[120, 123] = 37          # the reference's word stands where it is positive
    occ[0, 0] = 5
    nav = tr.nav_grid(occ, hits, passes)
    assert nav[120, 123] == 37 and nav[0, 0] == 5
    assert nav[120, 124] == 100 and nav[120, 121] == 0 and nav[120, 120] == 33 and nav[7, 7] == -1
    # the rounding: (100 h + (h + p) / 2) / (h + p) in integers
    assert tr.nav_grid(np.zeros(3, np.int8), [1, 1, 2], [1, 2, 1]).tolist() == [50, 33, 67]
    assert tr.nav_grid(np.zeros(1, np.int8), [0xffffffff], [2 ** 62]).tolist() == [0]


def steps_equal(xy, pose, cnt):
    return tr.steps_of(xy, pose, math.cos(pose[2]), math.sin(pose[2]), 60, 60, 0.25) == (cnt.n_rays, cnt.n_skipped, cnt.n_steps)


def test_trace_check_builds():
    from ndtpso_slam_amd import build
    build.build_hip()
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "host"), "libndtpso_slam.so", "replay/trace_check"], stdout=subprocess.DEVNULL)
    exe = os.path.join(ROOT, "host", "replay", "trace_check")
    assert os.access(exe, os.X_OK)
    assert subprocess.run([exe], stderr=subprocess.DEVNULL).returncode == 2       # usage: no arguments, nothing touched
    assert subprocess.run([exe, "--host-trace"], stderr=subprocess.DEVNULL).returncode == 2
    for recipe in ("Makefile", "CMakeLists.txt"):                                  # named as often as curvature_check is
        text = open(os.path.join(ROOT, "host", recipe)).read()
        assert text.count("trace_check") == text.count("curvature_check") > 0, recipe
