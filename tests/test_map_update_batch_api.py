"""CPU side of ndtpso_points_load_scans / ndtpso_map_update_batch (the scan loads and the map updates of several single calls in
shared launches) and of their C++ faces NDTFrame::loadLaserBatch / updateBatch: the exports and their bindings, the job structs'
layout, argument checks that need no device, and -- through replay/node_fleet, whose step is now one loadLaserBatch, one
alignBatch and one updateBatch -- the drop-in's failure semantics when there is no device at all."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "host")


def test_exports_and_bindings():
    from ndtpso_slam_amd import capi
    L = capi.load()
    for name in ("ndtpso_points_load_scans", "ndtpso_map_update_batch"):
        assert name in capi.EXPORTS and hasattr(L, name), name
    assert callable(capi.load_scans) and callable(capi.update_maps)


def test_job_struct_layouts_match_the_header():
    from ndtpso_slam_amd import capi
    src = open(os.path.join(ROOT, "include", "ndtpso_hip.h")).read()

    def define(name):
        m = re.search(r"#define %s (\d+)" % name, src)
        assert m, name
        return int(m.group(1))

    for struct in ("ndtpso_points_load_job", "ndtpso_map_update_job"):
        assert "static_assert(sizeof(%s) == %s_BYTES" % (struct, struct.upper()) in src
        assert "_Static_assert(sizeof(%s) == %s_BYTES" % (struct, struct.upper()) in src
    assert C.sizeof(capi.PointsLoadJob) == define("NDTPSO_POINTS_LOAD_JOB_BYTES")
    assert C.sizeof(capi.MapUpdateJob) == define("NDTPSO_MAP_UPDATE_JOB_BYTES")
    # the out fields where the header puts them
    assert capi.PointsLoadJob.rc.offset == define("NDTPSO_POINTS_LOAD_JOB_RC_OFFSET")
    assert capi.MapUpdateJob.rc.offset == define("NDTPSO_MAP_UPDATE_JOB_RC_OFFSET")
    assert capi.MapUpdateJob.route.offset == define("NDTPSO_MAP_UPDATE_JOB_ROUTE_OFFSET")
    # ... and the in fields in the header's order
    assert [f[0] for f in capi.PointsLoadJob._fields_] == ["pts", "ranges", "trans", "clip", "geom", "flags", "rc", "reserved"]
    assert [f[0] for f in capi.MapUpdateJob._fields_] == ["map", "points", "pose", "flags", "rc", "route", "reserved"]


def test_argument_checks_need_no_device():
    from ndtpso_slam_amd import capi
    L = capi.load()
    loads = (capi.PointsLoadJob * 2)()
    updates = (capi.MapUpdateJob * 2)()
    for fn, jobs in ((L.ndtpso_points_load_scans, loads), (L.ndtpso_map_update_batch, updates)):
        assert fn(None, jobs, 2) == capi.E_ARG          # null context
        assert fn(None, None, 2) == capi.E_ARG          # null jobs
        assert fn(None, jobs, 0) == capi.E_ARG          # no jobs
        assert fn(None, None, 0) == capi.E_ARG


def _scan_file(path, n_scans):
    from ndtpso_slam_amd import synth
    s = np.linspace(0.0, 0.3, n_scans)
    poses = np.stack([2.0 + 1.2 * s, -1.0 + 0.8 * np.sin(1.5 * s), 0.3 + 0.25 * s], axis=1)
    ranges = synth.raycast(poses).astype(np.float32)
    with open(path, "wb") as f:
        np.array([n_scans, synth.N_BEAMS], dtype=np.int32).tofile(f)
        np.array([synth.ANGLE_MIN, synth.ANGLE_INC, synth.RANGE_MAX], dtype=np.float32).tofile(f)
        ranges.tofile(f)


def _lines(stderr, what):
    return [line for line in stderr.splitlines() if what in line]


def test_node_fleet_batches_every_phase_and_survives_a_missing_device(tmp_path):
    from ndtpso_slam_amd import build as hip_build
    hip_build.build_hip()
    subprocess.check_call(["make", "-C", HOST, "-s"])
    exe = os.path.join(HOST, "replay", "node_fleet")
    assert os.path.exists(exe) and os.path.exists(os.path.join(HOST, "replay", "update_batch_check"))
    out = subprocess.check_output(["nm", "-D", "--demangle", os.path.join(HOST, "libndtpso_slam.so")], text=True)
    assert "NDTFrame::updateBatch(" in out and "NDTFrame::loadLaserBatch(" in out
    scans = tmp_path / "scans.bin"
    _scan_file(scans, 4)
    env = {k: v for k, v in os.environ.items()
           if k not in ("NDTPSO_ABORT_ON_ERROR", "NODE_FLEET_SEQUENTIAL", "NODE_FLEET_LOAD", "NODE_FLEET_UPDATE")}
    env["NDTPSO_DEVICE"] = "99"
    runs = {}
    for name, extra in (("batch", {}), ("sequential", {"NODE_FLEET_SEQUENTIAL": "1"})):
        prefix = str(tmp_path / name)
        r = subprocess.run([exe, str(scans), "60", "0.5", "50", "30", "1", "3", prefix], text=True, capture_output=True,
                           env=dict(env, **extra), timeout=120)
        assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[-2000:])          # it did not abort
        for robot in range(3):
            lines = open("%s.%d.poses" % (prefix, robot)).read().strip().splitlines()
            assert len(lines) == 4
            for k, line in enumerate(lines):
                f = line.split()
                assert int(f[0]) == k and [float(v) for v in f[1:]] == [0.0, 0.0, 0.0], line   # the initial guess, every time
        assert '"failed_alignments": 9' in r.stdout, r.stdout                          # 3 robots x 3 aligned scans
        runs[name] = r
    assert '"load": "batch", "update": "batch"' in runs["batch"].stdout, runs["batch"].stdout
    assert '"load": "calls", "update": "calls"' in runs["sequential"].stdout, runs["sequential"].stdout
    for key in ("host_ms_load_mean", "host_ms_align_mean", "host_ms_update_mean"):
        assert key in runs["batch"].stdout
    # stderr names the refused updates: the same lines, batched or call by call
    refused = _lines(runs["batch"].stderr, "update after a failed align")
    assert refused and refused == _lines(runs["sequential"].stderr, "update after a failed align"), runs["batch"].stderr[-2000:]
    assert "align failed" in runs["batch"].stderr
